// Host-side check of the code meter bank's C-ABI entries that need no device: rfa_code_word (the
// known answers of the DCS word), rfa_code_subcell (0, sub-cell boundaries, the 2^48 limit),
// rfa_code_merge (the carry over random cuts of a stream) and every argument error of rfa_code_*
// that returns before any HIP call.
// Built together with rfanalyzer_amd/csrc/code.hip with the host compiled under
// AddressSanitizer and UBSan (tools/Makefile) and run as an ordinary program;
// exits 0 when every check holds.
#include <cstdint>
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

static const int kCodes[] = {
    0023, 0025, 0026, 0031, 0032, 0036, 0043, 0047, 0051, 0053, 0054, 0065, 0071, 0072, 0073, 0074, 0114, 0115,
    0116, 0122, 0125, 0131, 0132, 0134, 0143, 0145, 0152, 0155, 0156, 0162, 0165, 0172, 0174, 0205, 0212, 0223,
    0225, 0226, 0243, 0244, 0245, 0246, 0251, 0252, 0255, 0261, 0263, 0265, 0266, 0271, 0274, 0306, 0311, 0315,
    0325, 0331, 0332, 0343, 0346, 0351, 0356, 0364, 0365, 0371, 0411, 0412, 0413, 0423, 0431, 0432, 0445, 0446,
    0452, 0454, 0455, 0462, 0464, 0465, 0466, 0503, 0506, 0516, 0523, 0526, 0532, 0546, 0565, 0606, 0612, 0624,
    0627, 0631, 0632, 0654, 0662, 0664, 0703, 0712, 0723, 0731, 0732, 0734, 0743, 0754};
static const int kNumCodes = (int)(sizeof(kCodes) / sizeof(kCodes[0]));

static uint32_t word_of(int code) {
    uint32_t w = 0;
    CHECK(rfa_code_word(code, &w) == RFA_OK);
    return w;
}

static bool is_rotation(uint32_t a, uint32_t b) {
    for (int r = 0; r < 23; r++)
        if ((((a >> r) | (a << (23 - r))) & 0x7fffffu) == b) return true;
    return false;
}

static void check_word() {
    CHECK(kNumCodes == 104);
    const uint32_t w023 = word_of(0023);
    CHECK(w023 == 0x763813u);
    CHECK(is_rotation(w023, word_of(0340)) && is_rotation(w023, word_of(0766)));
    const uint32_t inv = w023 ^ 0x7fffffu;
    CHECK(is_rotation(inv, word_of(0047)) && is_rotation(inv, word_of(0375)) && is_rotation(inv, word_of(0707)));
    for (int i = 0; i < kNumCodes; i++) {
        const uint32_t w = word_of(kCodes[i]);
        const int weight = __builtin_popcount(w);
        CHECK(weight == 11 || weight == 12);
        CHECK((w & 0xfffu) == (0x800u | (uint32_t)kCodes[i]) && w < (1u << 23));
        for (int j = 0; j < i; j++) CHECK(!is_rotation(w, word_of(kCodes[j])));
    }
    uint32_t w = 9;
    CHECK(rfa_code_word(-1, &w) == RFA_ERR_INVALID && rfa_code_word(512, &w) == RFA_ERR_INVALID && w == 9);
    CHECK(rfa_code_word(INT32_MIN, &w) == RFA_ERR_INVALID && rfa_code_word(INT32_MAX, &w) == RFA_ERR_INVALID);
    CHECK(rfa_code_word(0023, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_code_word(0, &w) == RFA_OK && (w & 0xfffu) == 0x800u);
    CHECK(rfa_code_word(0777, &w) == RFA_OK && (w & 0xfffu) == 0x9ffu);
}

static void check_subcell() {
    const __int128 num = 672 * RFA_CODE_SUBCELLS;
    const int64_t limit = (int64_t)1 << 48;
    for (int32_t rate : {RFA_CODE_MIN_RATE, 44100, 48000, RFA_CODE_MAX_RATE}) {
        const __int128 den = 5 * (__int128)rate;
        int64_t j = -9;
        CHECK(rfa_code_subcell(rate, 0, &j) == RFA_OK && j == 0);
        // either side of a sub-cell's first sample: ceil(c * den / num)
        for (int64_t c : {(int64_t)1, (int64_t)2, (int64_t)8, (int64_t)1000, (int64_t)123456789,
                          (int64_t)(num * limit / den)}) {
            const int64_t first = (int64_t)((c * den + num - 1) / num);
            CHECK(rfa_code_subcell(rate, first, &j) == RFA_OK && j == c);
            CHECK(rfa_code_subcell(rate, first - 1, &j) == RFA_OK && j == c - 1);
        }
        for (int64_t g : {(int64_t)1, (int64_t)44, (int64_t)45, (int64_t)1 << 31, limit - 1, limit}) {
            CHECK(rfa_code_subcell(rate, g, &j) == RFA_OK);
            CHECK(j == (int64_t)(num * g / den));            // in 128 bits: the product did not wrap in 64
        }
        j = -9;
        CHECK(rfa_code_subcell(rate, -1, &j) == RFA_ERR_INVALID);
        CHECK(rfa_code_subcell(rate, limit + 1, &j) == RFA_ERR_INVALID);
        CHECK(rfa_code_subcell(rate, INT64_MAX, &j) == RFA_ERR_INVALID);
        CHECK(rfa_code_subcell(rate, INT64_MIN, &j) == RFA_ERR_INVALID);
        CHECK(rfa_code_subcell(rate, 0, nullptr) == RFA_ERR_INVALID);
        CHECK(j == -9);
    }
    int64_t j = -9;
    for (int32_t rate : {RFA_CODE_MIN_RATE - 1, RFA_CODE_MAX_RATE + 1, 0, -48000, INT32_MIN, INT32_MAX})
        CHECK(rfa_code_subcell(rate, 0, &j) == RFA_ERR_INVALID && j == -9);
    // at 48 kHz a sub-cell holds 44 or 45 samples
    int64_t prev = 0, run = 0;
    for (int64_t g = 0; g < 48000; g++) {
        CHECK(rfa_code_subcell(48000, g, &j) == RFA_OK);
        if (j != prev) {
            CHECK(j == prev + 1 && (run == 44 || run == 45));
            prev = j;
            run = 0;
        }
        run++;
    }
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// A stream of per-sample integers cut into calls at random points, zero-length calls among them: the
// completed sub-cells that rfa_code_merge hands out, call after call, are those of the stream summed whole.
static void check_merge() {
    for (int32_t rate : {RFA_CODE_MIN_RATE, 48000}) {
        const int64_t n = 5000;
        std::vector<int64_t> q((size_t)n), cell((size_t)n);
        for (int64_t g = 0; g < n; g++) {
            q[(size_t)g] = (int64_t)(rng() % 2000001) - 1000000;
            CHECK(rfa_code_subcell(rate, g, &cell[(size_t)g]) == RFA_OK);
        }
        int64_t after = 0;
        CHECK(rfa_code_subcell(rate, n, &after) == RFA_OK);
        std::vector<int64_t> whole((size_t)cell.back() + 1, 0);
        for (int64_t g = 0; g < n; g++) whole[(size_t)cell[(size_t)g]] += q[(size_t)g];
        if (after == cell.back()) whole.pop_back();         // the last one is incomplete
        for (int trial = 0; trial < 50; trial++) {
            int32_t valid = 0;
            int64_t cj = 0, cs = 0, g = 0;
            std::vector<int64_t> got;
            while (g < n) {
                int64_t len = (int64_t)(rng() % 4 == 0 ? 0 : rng() % 700);
                if (g + len > n) len = n - g;
                int64_t j0 = 0;
                CHECK(rfa_code_subcell(rate, g, &j0) == RFA_OK);
                const int64_t m = len ? cell[(size_t)(g + len - 1)] - j0 + 1 : 0;
                std::vector<int64_t> sums((size_t)m, 0);
                for (int64_t i = g; i < g + len; i++) sums[(size_t)(cell[(size_t)i] - j0)] += q[(size_t)i];
                int64_t first = -9, count = -9;
                CHECK(rfa_code_merge(rate, g + len, j0, m, sums.data(), &valid, &cj, &cs, &first, &count) == RFA_OK);
                CHECK(first == j0 && count >= 0 && count <= m && (count == m || count == m - 1));
                if (count) CHECK(first == (int64_t)got.size());
                got.insert(got.end(), sums.begin(), sums.begin() + count);
                CHECK(!valid || (cj == j0 + m - 1 && count == m - 1) || m == 0);
                g += len;
            }
            CHECK(got == whole);
        }
    }
    int32_t valid = 1;
    int64_t cj = 5, cs = 7, first = -9, count = -9, sums[2] = {1, 2};
    CHECK(rfa_code_merge(48000, 300, 6, 2, sums, &valid, &cj, &cs, &first, &count) == RFA_ERR_INVALID);  // carry != j0
    CHECK(rfa_code_merge(48000, 300, 5, 2, nullptr, &valid, &cj, &cs, &first, &count) == RFA_ERR_INVALID);
    CHECK(rfa_code_merge(48000, 300, 5, 2, sums, nullptr, &cj, &cs, &first, &count) == RFA_ERR_INVALID);
    CHECK(rfa_code_merge(48000, 300, 5, 2, sums, &valid, nullptr, &cs, &first, &count) == RFA_ERR_INVALID);
    CHECK(rfa_code_merge(48000, 300, 5, 2, sums, &valid, &cj, nullptr, &first, &count) == RFA_ERR_INVALID);
    CHECK(rfa_code_merge(48000, 300, 5, 2, sums, &valid, &cj, &cs, nullptr, &count) == RFA_ERR_INVALID);
    CHECK(rfa_code_merge(48000, 300, 5, 2, sums, &valid, &cj, &cs, &first, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_code_merge(7999, 300, 5, 2, sums, &valid, &cj, &cs, &first, &count) == RFA_ERR_INVALID);
    CHECK(rfa_code_merge(48000, -1, 5, 2, sums, &valid, &cj, &cs, &first, &count) == RFA_ERR_INVALID);
    CHECK(rfa_code_merge(48000, ((int64_t)1 << 48) + 1, 5, 2, sums, &valid, &cj, &cs, &first, &count) ==
          RFA_ERR_INVALID);
    CHECK(rfa_code_merge(48000, 300, -1, 2, sums, &valid, &cj, &cs, &first, &count) == RFA_ERR_INVALID);
    CHECK(rfa_code_merge(48000, 300, 5, -1, sums, &valid, &cj, &cs, &first, &count) == RFA_ERR_INVALID);
    CHECK(valid == 1 && cj == 5 && cs == 7 && sums[0] == 1 && sums[1] == 2);
    // no samples: the carry stays; NULL sums are fine then
    CHECK(rfa_code_merge(48000, 300, 5, 0, nullptr, &valid, &cj, &cs, &first, &count) == RFA_OK);
    CHECK(valid == 1 && cj == 5 && cs == 7 && first == 5 && count == 0);
}

static void check_create_errors() {
    rfa_code *t = reinterpret_cast<rfa_code *>(0x1);
    CHECK(rfa_code_create(0, 4, 48000, nullptr) == RFA_ERR_INVALID);
    for (int32_t k : {0, -1, RFA_CODE_MAX_CHANNELS + 1, INT32_MIN, INT32_MAX}) {
        t = reinterpret_cast<rfa_code *>(0x1);
        CHECK(rfa_code_create(0, k, 48000, &t) == RFA_ERR_INVALID && t == nullptr);
    }
    for (int32_t rate : {RFA_CODE_MIN_RATE - 1, RFA_CODE_MAX_RATE + 1, 0, -1, INT32_MIN, INT32_MAX}) {
        t = reinterpret_cast<rfa_code *>(0x1);
        CHECK(rfa_code_create(0, 4, rate, &t) == RFA_ERR_INVALID && t == nullptr);
    }
    // valid requests: the device is looked for only now (this program runs where there is none)
    for (int32_t k : {1, 32, RFA_CODE_MAX_CHANNELS}) {
        t = reinterpret_cast<rfa_code *>(0x1);
        const int st = rfa_code_create(0, k, RFA_CODE_MIN_RATE, &t);
        CHECK(st == RFA_ERR_NODEVICE || st == RFA_OK);
        CHECK(st == RFA_OK || t == nullptr);
        if (st == RFA_OK && t) CHECK(rfa_code_destroy(t) == RFA_OK);
    }
}

static void check_null_handle() {
    CHECK(rfa_code_destroy(nullptr) == RFA_ERR_INVALID);
    CHECK(std::strcmp(rfa_code_last_error(nullptr), "null handle") == 0);
    int32_t w[2] = {9, 9};
    int64_t d[8];
    for (int64_t &v : d) v = 9;
    size_t cnt[2] = {2, 2};
    float x[4] = {9.0f, 9.0f, 9.0f, 9.0f};
    void *st = nullptr;
    CHECK(rfa_code_get_channels(nullptr, w, w + 1) == RFA_ERR_INVALID);
    CHECK(rfa_code_get_channels(nullptr, nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_code_break(nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_code_break(nullptr, -1) == RFA_ERR_INVALID);
    CHECK(rfa_code_reset(nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_code_process(nullptr, x, 2, cnt) == RFA_ERR_INVALID);
    CHECK(rfa_code_process(nullptr, nullptr, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_code_collect(nullptr, d, d + 2, d + 4, 2, d + 6, d + 7) == RFA_ERR_INVALID);
    CHECK(rfa_code_collect(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_code_process_host(nullptr, x, 2, cnt, d, d + 2, d + 4, 1, d + 6, d + 7) == RFA_ERR_INVALID);
    CHECK(rfa_code_set_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_code_get_stream(nullptr, &st) == RFA_ERR_INVALID);
    CHECK(rfa_code_get_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_code_synchronize(nullptr) == RFA_ERR_INVALID);
    // nothing written through a null handle
    CHECK(w[0] == 9 && w[1] == 9 && d[0] == 9 && d[7] == 9 && x[0] == 9.0f);
}

// With a device (not where the test suite runs this): the argument errors of a live handle.
static void check_live_errors() {
    rfa_code *t = nullptr;
    if (rfa_code_create(0, 2, RFA_CODE_MIN_RATE, &t) != RFA_OK) return;
    float x[8] = {};
    int64_t first[2], count[2], bad[2], n[2], sums[8];
    int32_t w = 0, rate = 0;
    size_t cnt[2] = {2, 2};
    CHECK(rfa_code_get_channels(t, &w, &rate) == RFA_OK && w == 2 && rate == RFA_CODE_MIN_RATE);
    CHECK(rfa_code_get_channels(t, nullptr, &rate) == RFA_ERR_INVALID);
    CHECK(rfa_code_break(t, 2) == RFA_ERR_INVALID);
    CHECK(rfa_code_break(t, -2) == RFA_ERR_INVALID);
    CHECK(rfa_code_process(t, nullptr, 4, cnt) == RFA_ERR_INVALID);
    CHECK(rfa_code_process(t, x, 4, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_code_process(t, x, 1, cnt) == RFA_ERR_INVALID);              // a count above the stride
    cnt[1] = ((size_t)1 << 36) + 1;
    CHECK(rfa_code_process(t, x, (size_t)1 << 37, cnt) == RFA_ERR_INVALID);
    cnt[1] = 2;
    CHECK(rfa_code_process_host(t, x, 1, cnt, first, count, sums, 4, bad, n) == RFA_ERR_INVALID);
    CHECK(rfa_code_process_host(t, nullptr, 4, cnt, first, count, sums, 4, bad, n) == RFA_ERR_INVALID);
    CHECK(rfa_code_collect(t, first, count, sums, 4, bad, n) == RFA_OK && count[0] == 0 && count[1] == 0 && n[1] == 0);
    CHECK(rfa_code_destroy(t) == RFA_OK);
}

int main() {
    check_word();
    check_subcell();
    check_merge();
    check_create_errors();
    check_null_handle();
    check_live_errors();
    if (failures) {
        std::fprintf(stderr, "code_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("code_host_check ok\n");
    return 0;
}
