// Host-side check of the audio IIR bank's C-ABI entries that need no device: rfa_audio_iir_tables
// (against the recurrence written out here, and the stability triangle's edges),
// rfa_audio_iir_plan, rfa_audio_iir_carry_after, and every argument error of rfa_audio_iir_* that
// returns before any HIP call; with a device also the section round trips and the argument errors
// of a live handle.
// Built together with rfanalyzer_amd/csrc/audio_iir.hip with the host compiled under
// AddressSanitizer and UBSan (tools/Makefile) and run as an ordinary program;
// exits 0 when every check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/rfa.h"

#pragma clang fp contract(off)

static int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static const int B = RFA_AUDIO_IIR_BLOCK;
static const int NB = RFA_AUDIO_IIR_CHUNK_BLOCKS;
static const size_t kMaxCount = (size_t)1 << 36;
static const float kInf = std::numeric_limits<float>::infinity();

// a Chebyshev II pair, a Butterworth pair, a one-pole, a notch with its poles at 0.999
static const float kSections[4][5] = {{0.9952473f, -1.989428f, 0.9952473f, -1.9891472f, 0.9907755f},
                                      {0.97f, -1.94f, 0.97f, -1.94f, 0.9416f},
                                      {0.027f, 0.0f, 0.0f, -0.973f, 0.0f},
                                      {0.999f, -1.981f, 0.999f, -1.9810f, 0.998001f}};

static void check_tables() {
    std::vector<float> G(2 * (size_t)B + 1, -9.0f);
    float P[5] = {-9.0f, -9.0f, -9.0f, -9.0f, -9.0f};
    for (const float *c : {kSections[0], kSections[1], kSections[2], kSections[3]}) {
        CHECK(rfa_audio_iir_tables(c[3], c[4], G.data(), P) == RFA_OK);
        CHECK(G[2 * (size_t)B] == -9.0f && P[4] == -9.0f);          // nothing behind the tables
        CHECK(G[0] == 1.0f && G[1] == 0.0f && G[2] == -c[3] && G[3] == 1.0f);
        // R_{i+1} = R_i A in double, the first row handed out as G[i], R_B as P
        const double a1 = c[3], a2 = c[4];
        double R[2][2] = {{1.0, 0.0}, {0.0, 1.0}};
        for (int i = 0; i < B; i++) {
            CHECK(G[2 * (size_t)i] == (float)R[0][0] && G[2 * (size_t)i + 1] == (float)R[0][1]);
            for (int r = 0; r < 2; r++) {
                const double x0 = R[r][0], x1 = R[r][1];
                R[r][0] = (x0 * -a1) + (x1 * -a2);
                R[r][1] = (x0 * 1.0) + (x1 * 0.0);
            }
        }
        CHECK(P[0] == (float)R[0][0] && P[1] == (float)R[0][1] && P[2] == (float)R[1][0] && P[3] == (float)R[1][1]);
        for (float v : G) CHECK(std::isfinite(v));
    }
    // the stability triangle: |a2| < 1 and |a1| < 1 + a2, its edges outside
    const float below1 = std::nextafterf(1.0f, 0.0f);
    const struct { float a1, a2; bool ok; } cases[] = {
        {0.0f, 0.0f, true},      {0.0f, below1, true},    {0.0f, 1.0f, false},       {0.0f, -1.0f, false},
        {0.0f, -below1, true},   {1.0f, 0.0f, false},     {-1.0f, 0.0f, false},      {below1, 0.0f, true},
        {-below1, 0.0f, true},   {1.5f, 0.5f, false},     {-1.5f, 0.5f, false},      {1.49f, 0.5f, true},
        {-1.49f, 0.5f, true},    {2.0f, 1.0f, false},     {0.5f, -0.5f, false},      {0.49f, -0.5f, true},
        {kInf, 0.0f, false},     {0.0f, -kInf, false},    {std::nanf(""), 0.0f, false}, {0.0f, std::nanf(""), false}};
    for (const auto &t : cases) {
        std::fill(G.begin(), G.end(), -9.0f);
        for (float &v : P) v = -9.0f;
        CHECK((rfa_audio_iir_tables(t.a1, t.a2, G.data(), P) == RFA_OK) == t.ok);
        if (!t.ok) CHECK(G[0] == -9.0f && G[2 * (size_t)B - 1] == -9.0f && P[0] == -9.0f && P[3] == -9.0f);
    }
    CHECK(rfa_audio_iir_tables(0.0f, 0.0f, nullptr, P) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_tables(0.0f, 0.0f, G.data(), nullptr) == RFA_ERR_INVALID);
}

static void check_plan_and_carry() {
    int32_t p[RFA_AUDIO_IIR_PLAN_FIELDS];
    const size_t C = (size_t)NB * B;
    const size_t counts[] = {0, 1, 127, 128, 129, C - 1, C, C + 1, 2 * C + 5, 335544, kMaxCount};
    for (int32_t S : {0, 1, 4, 5, RFA_AUDIO_IIR_MAX_SECTIONS})
        for (size_t n : counts)
            for (int32_t a : {0, 1, 127}) {
                for (int32_t &v : p) v = -9;
                CHECK(rfa_audio_iir_plan(S, n, a, p) == RFA_OK);
                const size_t touched = n ? ((size_t)a + n + B - 1) / B : 0;
                const bool work = n && S;
                CHECK(p[0] == B && p[1] == NB);
                CHECK(p[3] == (n == 0 ? RFA_AUDIO_IIR_PATH_NONE : S == 0 ? RFA_AUDIO_IIR_PATH_COPY : RFA_AUDIO_IIR_PATH_BLOCKED));
                CHECK((size_t)p[5] == touched);
                CHECK((size_t)p[4] == (work ? (touched + NB - 1) / NB : 0));
                if (work) {
                    const size_t nb = touched < (size_t)NB ? touched : (size_t)NB;
                    CHECK((size_t)p[2] >= sizeof(float) * nb * ((size_t)B + 1 + 4));   // rows at stride B + 1, z_end, s0
                    CHECK(p[2] <= 160 * 1024);                                           // the LDS of a compute unit
                } else {
                    CHECK(p[2] == 0);
                }
                int32_t next = -9;
                CHECK(rfa_audio_iir_carry_after(n, a, &next) == RFA_OK);
                CHECK((size_t)next == ((size_t)a + n) % B);
            }
    for (int32_t &v : p) v = -9;
    int32_t next = -9;
    CHECK(rfa_audio_iir_plan(-1, 10, 0, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_plan(RFA_AUDIO_IIR_MAX_SECTIONS + 1, 10, 0, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_plan(INT32_MIN, 10, 0, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_plan(INT32_MAX, 10, 0, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_plan(4, kMaxCount + 1, 0, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_plan(4, SIZE_MAX, 0, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_plan(4, 10, -1, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_plan(4, 10, B, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_plan(4, 10, INT32_MIN, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_plan(4, 10, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_carry_after(10, -1, &next) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_carry_after(10, B, &next) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_carry_after(10, INT32_MAX, &next) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_carry_after(kMaxCount + 1, 0, &next) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_carry_after(SIZE_MAX, 0, &next) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_carry_after(10, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(p[0] == -9 && p[5] == -9 && next == -9);
}

static void check_create_errors() {
    rfa_audio_iir *f = reinterpret_cast<rfa_audio_iir *>(0x1);
    CHECK(rfa_audio_iir_create(0, 4, nullptr) == RFA_ERR_INVALID);
    for (int32_t k : {0, -1, RFA_AUDIO_IIR_MAX_CHANNELS + 1, INT32_MIN, INT32_MAX}) {
        f = reinterpret_cast<rfa_audio_iir *>(0x1);
        CHECK(rfa_audio_iir_create(0, k, &f) == RFA_ERR_INVALID && f == nullptr);
    }
    // valid requests: the device is looked for only now
    for (int32_t k : {1, 32, RFA_AUDIO_IIR_MAX_CHANNELS}) {
        f = reinterpret_cast<rfa_audio_iir *>(0x1);
        const int st = rfa_audio_iir_create(0, k, &f);
        CHECK(st == RFA_ERR_NODEVICE || st == RFA_OK);
        CHECK(st == RFA_OK || f == nullptr);
        if (st == RFA_OK && f) CHECK(rfa_audio_iir_destroy(f) == RFA_OK);
    }
}

static void check_null_handle() {
    CHECK(rfa_audio_iir_destroy(nullptr) == RFA_ERR_INVALID);
    CHECK(std::strcmp(rfa_audio_iir_last_error(nullptr), "null handle") == 0);
    int32_t w = 9;
    size_t cnt[2] = {2, 2};
    float x[5] = {9.0f, 9.0f, 9.0f, 9.0f, 9.0f}, y[5] = {9.0f, 9.0f, 9.0f, 9.0f, 9.0f};
    void *st = nullptr;
    CHECK(rfa_audio_iir_get_channels(nullptr, &w) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_get_channels(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_set_sections(nullptr, 0, kSections[0], 1) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_set_sections(nullptr, 0, nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_get_sections(nullptr, 0, y, 1, &w) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_reset(nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_reset(nullptr, -1) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_process(nullptr, x, 2, cnt, y, 2) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_process(nullptr, nullptr, 0, nullptr, nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_process_host(nullptr, x, 2, cnt, y, 2) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_process_host(nullptr, nullptr, 0, nullptr, nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_set_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_get_stream(nullptr, &st) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_get_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_synchronize(nullptr) == RFA_ERR_INVALID);
    // nothing written through a null handle
    CHECK(w == 9 && y[0] == 9.0f && y[4] == 9.0f && x[0] == 9.0f);
}

// With a device: section round trips and the argument errors of a live handle.  A handle needs
// device memory; without one this part is skipped and says so.
static void check_live() {
    rfa_audio_iir *f = nullptr;
    if (rfa_audio_iir_create(0, 2, &f) != RFA_OK) {
        std::printf("audio_iir_host_check: no device, live-handle checks (section round trips, argument errors) skipped\n");
        return;
    }
    int32_t w = 0;
    CHECK(rfa_audio_iir_get_channels(f, &w) == RFA_OK && w == 2);
    CHECK(rfa_audio_iir_get_channels(f, nullptr) == RFA_ERR_INVALID);
    std::vector<float> sec(5 * (RFA_AUDIO_IIR_MAX_SECTIONS + 1)), got(5 * RFA_AUDIO_IIR_MAX_SECTIONS, -1.0f);
    for (size_t q = 0; q < sec.size() / 5; q++) std::memcpy(&sec[5 * q], kSections[q % 4], 5 * sizeof(float));
    for (int32_t S : {0, 1, RFA_AUDIO_IIR_MAX_SECTIONS, 1, 0}) {
        CHECK(rfa_audio_iir_set_sections(f, 1, sec.data(), S) == RFA_OK);
        int32_t n = -1;
        CHECK(rfa_audio_iir_get_sections(f, 1, nullptr, 0, &n) == RFA_OK && n == S);
        std::fill(got.begin(), got.end(), -1.0f);
        CHECK(rfa_audio_iir_get_sections(f, 1, got.data(), RFA_AUDIO_IIR_MAX_SECTIONS, &n) == RFA_OK && n == S);
        CHECK(std::memcmp(got.data(), sec.data(), (size_t)S * 5 * sizeof(float)) == 0);
        CHECK(S == RFA_AUDIO_IIR_MAX_SECTIONS || got[(size_t)S * 5] == -1.0f);
        CHECK(rfa_audio_iir_get_sections(f, 0, nullptr, 0, &n) == RFA_OK && n == 0);     // the other slot is untouched
    }
    {                                                      // a buffer too small: the count, and nothing copied
        int32_t n = -1;
        CHECK(rfa_audio_iir_set_sections(f, 1, sec.data(), 3) == RFA_OK);
        std::fill(got.begin(), got.end(), -1.0f);
        CHECK(rfa_audio_iir_get_sections(f, 1, got.data(), 2, &n) == RFA_ERR_INVALID && n == 3 && got[0] == -1.0f);
        CHECK(rfa_audio_iir_get_sections(f, 1, got.data(), 3, &n) == RFA_OK && n == 3 && got[0] == sec[0]);
    }
    CHECK(rfa_audio_iir_set_sections(f, 0, nullptr, 0) == RFA_OK);
    CHECK(rfa_audio_iir_set_sections(f, 0, nullptr, 3) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_set_sections(f, 2, sec.data(), 3) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_set_sections(f, -1, sec.data(), 3) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_set_sections(f, 0, sec.data(), -1) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_set_sections(f, 0, sec.data(), RFA_AUDIO_IIR_MAX_SECTIONS + 1) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_set_sections(f, 0, sec.data(), 2) == RFA_OK);
    for (int at = 0; at < 5; at++)
        for (float bad : {kInf, -kInf, std::nanf("")}) {
            float two[10];
            std::memcpy(two, sec.data(), sizeof(two));
            two[5 + at] = bad;
            int32_t n = -1;
            CHECK(rfa_audio_iir_set_sections(f, 0, two, 2) == RFA_ERR_INVALID);
            CHECK(rfa_audio_iir_get_sections(f, 0, got.data(), RFA_AUDIO_IIR_MAX_SECTIONS, &n) == RFA_OK && n == 2 &&
                  std::memcmp(got.data(), sec.data(), 10 * sizeof(float)) == 0);
        }
    const float unstable[3][5] = {{1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, {1.0f, 0.0f, 0.0f, 1.5f, 0.5f}, {1.0f, 0.0f, 0.0f, -1.0f, 0.0f}};
    for (const float *u : {unstable[0], unstable[1], unstable[2]}) CHECK(rfa_audio_iir_set_sections(f, 0, u, 1) == RFA_ERR_INVALID);
    int32_t n = 0;
    CHECK(rfa_audio_iir_get_sections(f, 2, got.data(), 8, &n) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_get_sections(f, 0, got.data(), 8, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_reset(f, 2) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_reset(f, -2) == RFA_ERR_INVALID);
    float *x = nullptr;                                    // never dereferenced: these calls fail their checks
    float dummy[16] = {};
    size_t cnt[2] = {2, 2}, zero[2] = {0, 0};
    CHECK(rfa_audio_iir_process(f, nullptr, 4, cnt, dummy, 4) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_process(f, dummy, 4, cnt, x, 4) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_process(f, dummy, 4, nullptr, dummy + 8, 4) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_process(f, dummy, 1, cnt, dummy + 8, 4) == RFA_ERR_INVALID);     // a count above in_stride
    CHECK(rfa_audio_iir_process(f, dummy, 4, cnt, dummy + 8, 1) == RFA_ERR_INVALID);     // ... above out_stride
    CHECK(rfa_audio_iir_process(f, dummy, 4, cnt, dummy, 4) == RFA_ERR_INVALID);         // in place
    CHECK(rfa_audio_iir_process(f, dummy, 4, cnt, dummy + 1, 4) == RFA_ERR_INVALID);     // overlapping
    CHECK(rfa_audio_iir_process(f, dummy, 4, cnt, dummy + 5, 4) == RFA_ERR_INVALID);     // row 1 of in, row 0 of out
    cnt[1] = kMaxCount + 1;
    CHECK(rfa_audio_iir_process(f, dummy, (size_t)1 << 37, cnt, dummy + 8, (size_t)1 << 37) == RFA_ERR_INVALID);
    CHECK(rfa_audio_iir_process(f, nullptr, 0, zero, nullptr, 0) == RFA_OK);             // no samples: nothing is looked at
    CHECK(rfa_audio_iir_process_host(f, nullptr, 0, zero, nullptr, 0) == RFA_OK);
    CHECK(rfa_audio_iir_destroy(f) == RFA_OK);
}

int main() {
    check_tables();
    check_plan_and_carry();
    check_create_errors();
    check_null_handle();
    check_live();
    if (failures) {
        std::fprintf(stderr, "audio_iir_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("audio_iir_host_check ok\n");
    return 0;
}
