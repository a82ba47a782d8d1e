// Host-side check of the audio resampler bank's C-ABI entries that need no device:
// rfa_audio_rs_counts (the call rule, walked in random splits against one whole call and against its
// closed form, for every ratio of the device tests' case table and n up to 2^36),
// rfa_audio_rs_max_outputs, rfa_audio_rs_plan, and every argument error of rfa_audio_rs_* that
// returns before any HIP call.
// Built together with rfanalyzer_amd/csrc/audio_rs.hip with the host compiled under
// AddressSanitizer and UBSan (tools/Makefile) and run as an ordinary program;
// exits 0 when every check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
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

static const size_t kMaxCount = (size_t)1 << 36;

struct Ratio {
    int32_t L, D;
};
// the ratios of tests/audio_rs_paths.py and the corners of the limits
static const Ratio kRatios[] = {{1, 1}, {1, 2}, {1, 3}, {1, 6}, {2, 3}, {147, 160}, {147, 640},
                                {1, 1024}, {160, 1023}, {159, 160}, {1, 7}};
static const Ratio kBadRatios[] = {{0, 1}, {-1, 6}, {161, 640}, {2, 1}, {1, 1025}, {2, 4}, {147, 147}, {6, 9},
                                   {INT32_MAX, INT32_MAX}, {INT32_MIN, 6}, {1, INT32_MIN}};

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {                                    // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}

static void check_counts() {
    for (const Ratio q : kRatios) {
        const unsigned __int128 L = (unsigned)q.L, D = (unsigned)q.D;
        const size_t counts[] = {0, 1, 2, (size_t)q.D - 1, (size_t)q.D, (size_t)q.D + 1, 12345, ((size_t)1 << 31) + 11,
                                 kMaxCount - 1, kMaxCount};
        for (size_t n : counts)
            for (int32_t r : {0, q.D / 2, q.D - 1}) {
                size_t m = 99;
                int32_t rn = -9;
                CHECK(rfa_audio_rs_counts(q.L, q.D, r, n, &m, &rn) == RFA_OK);
                // the closed form, in 128 bits
                const unsigned __int128 ticks = (unsigned __int128)n * L;
                const unsigned __int128 want = ticks > (unsigned)r ? (ticks - (unsigned)r + D - 1) / D : 0;
                CHECK((unsigned __int128)m == want);
                CHECK(rn >= 0 && rn < q.D);
                CHECK((unsigned __int128)(unsigned)rn + ticks == (unsigned)r + want * D);
                // the rule in its own words: outputs while r + m D < n L
                CHECK(m == 0 || (unsigned)r + (want - 1) * D < ticks);
                CHECK((unsigned)r + want * D >= ticks);
            }
        for (size_t n : counts) CHECK((unsigned __int128)rfa_audio_rs_max_outputs(q.L, q.D, n) == ((unsigned __int128)n * L + D - 1) / D);
        // a stream cut anywhere gives the whole stream's count and final offset
        for (size_t total : {(size_t)1000, (size_t)1 << 20, kMaxCount}) {
            size_t whole = 0;
            int32_t r_whole = -1;
            CHECK(rfa_audio_rs_counts(q.L, q.D, 0, total, &whole, &r_whole) == RFA_OK);
            for (int trial = 0; trial < 8; trial++) {
                size_t left = total, outs = 0;
                int32_t r = 0;
                for (int piece = 0; piece < 9 && left; piece++) {
                    const size_t n = piece == 8 ? left : (size_t)(rng() % (left + 1)) >> (rng() % 3 ? 0 : 20);
                    size_t m = 0;
                    int32_t rn = -1;
                    CHECK(rfa_audio_rs_counts(q.L, q.D, r, n, &m, &rn) == RFA_OK);
                    outs += m;
                    r = rn;
                    left -= n;
                }
                if (left) {
                    size_t m = 0;
                    int32_t rn = -1;
                    CHECK(rfa_audio_rs_counts(q.L, q.D, r, left, &m, &rn) == RFA_OK);
                    outs += m;
                    r = rn;
                }
                CHECK(outs == whole && r == r_whole);
            }
        }
    }
    size_t m = 77;
    int32_t rn = 77;
    for (const Ratio q : kBadRatios) {
        CHECK(rfa_audio_rs_counts(q.L, q.D, 0, 10, &m, &rn) == RFA_ERR_INVALID);
        CHECK(rfa_audio_rs_max_outputs(q.L, q.D, 10) == 0);
    }
    for (int32_t r : {-1, 6, INT32_MAX, INT32_MIN}) CHECK(rfa_audio_rs_counts(1, 6, r, 10, &m, &rn) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_counts(1, 6, 0, kMaxCount + 1, &m, &rn) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_counts(1, 6, 0, SIZE_MAX, &m, &rn) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_counts(1, 6, 0, 10, nullptr, &rn) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_counts(1, 6, 0, 10, &m, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_max_outputs(1, 6, kMaxCount + 1) == 0);
    CHECK(rfa_audio_rs_max_outputs(1, 6, SIZE_MAX) == 0);
    CHECK(m == 77 && rn == 77);
}

struct Shape {
    int32_t L, D, T;
};

static void check_plan() {
    static const Shape shapes[] = {{1, 1, 0}, {1, 1, 5}, {1, 2, 4096}, {1, 3, 65}, {1, 6, 219}, {2, 3, 1}, {2, 3, 7},
                                   {2, 3, 8}, {147, 160, 100}, {147, 160, 1000}, {147, 640, 1176}, {147, 640, 16384},
                                   {1, 1024, 4096}, {1, 1024, 1}, {160, 1023, 16384}, {2, 1023, 8192}};
    int32_t p[RFA_AUDIO_RS_PLAN_FIELDS];
    for (const Shape s : shapes) {
        for (int32_t &v : p) v = -9;
        CHECK(rfa_audio_rs_plan(s.L, s.D, s.T, 1, p) == RFA_OK);
        const int32_t tile = p[0];
        CHECK(tile >= 1 && tile <= RFA_AUDIO_RS_MAX_TILE && (tile & (tile - 1)) == 0);
        const int32_t J = (s.T + s.L - 1) / s.L;
        const size_t tile_in = (size_t)tile * (size_t)s.D / (size_t)s.L;
        const size_t counts[] = {0, 1, (size_t)s.D, tile_in - 1, tile_in, tile_in + 1, 3 * tile_in, kMaxCount};
        for (size_t n : counts) {
            for (int32_t &v : p) v = -9;
            CHECK(rfa_audio_rs_plan(s.L, s.D, s.T, n, p) == RFA_OK);
            const size_t n_out = rfa_audio_rs_max_outputs(s.L, s.D, n);
            const int path = n == 0 ? RFA_AUDIO_RS_PATH_NONE
                             : s.T == 0 ? RFA_AUDIO_RS_PATH_CONVERT
                             : s.L == 1 ? RFA_AUDIO_RS_PATH_DECIMATE
                                        : RFA_AUDIO_RS_PATH_POLYPHASE;
            CHECK(p[0] == tile && p[2] == path);
            const size_t groups = (n_out + (size_t)tile - 1) / (size_t)tile;
            CHECK((size_t)p[4] == (groups < (size_t)INT32_MAX ? groups : (size_t)INT32_MAX));
            const size_t in_tile = n_out < (size_t)tile ? n_out : (size_t)tile;
            CHECK((size_t)p[3] * 256 >= in_tile && (p[3] == 0) == (n == 0));
            CHECK(p[3] == 0 || p[3] == 1 || p[3] == 2 || p[3] == 4);
            if (n == 0 || s.T == 0) {
                CHECK(p[1] == 0);
            } else {
                // the taps of every phase, and the tile's inputs with J - 1 before them
                const size_t span = ((size_t)(s.L - 1) + (size_t)(tile - 1) * (size_t)s.D) / (size_t)s.L + (size_t)J;
                CHECK(p[1] % 16 == 0);
                CHECK((size_t)p[1] >= sizeof(float) * ((size_t)s.L * (size_t)J + span));
                CHECK(p[1] <= 160 * 1024);                 // a CU's LDS
            }
        }
    }
    for (int32_t &v : p) v = -9;
    for (const Ratio q : kBadRatios) CHECK(rfa_audio_rs_plan(q.L, q.D, 4, 10, p) == RFA_ERR_INVALID);
    static const Shape bad[] = {{1, 6, 0}, {2, 3, 0}, {1, 1, -1}, {1, 6, 4097}, {2, 3, 8193}, {147, 640, 16385},
                                {1, 1, INT32_MAX}, {1, 1, INT32_MIN}};
    for (const Shape s : bad) CHECK(rfa_audio_rs_plan(s.L, s.D, s.T, 10, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_plan(1, 6, 4, kMaxCount + 1, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_plan(1, 6, 4, SIZE_MAX, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_plan(1, 6, 4, 10, nullptr) == RFA_ERR_INVALID);
    CHECK(p[0] == -9 && p[4] == -9);
}

static void check_create_errors() {
    std::vector<float> taps(RFA_AUDIO_RS_MAX_TAPS + 1, 0.001f);
    rfa_audio_rs *s = reinterpret_cast<rfa_audio_rs *>(0x1);
    CHECK(rfa_audio_rs_create(0, 4, 1, 6, taps.data(), 7, nullptr) == RFA_ERR_INVALID);
    auto refused = [&](int32_t k, int32_t L, int32_t D, const float *t, int32_t T) {
        s = reinterpret_cast<rfa_audio_rs *>(0x1);
        return rfa_audio_rs_create(0, k, L, D, t, T, &s) == RFA_ERR_INVALID && s == nullptr;
    };
    for (int32_t k : {0, -1, RFA_AUDIO_RS_MAX_CHANNELS + 1, INT32_MIN, INT32_MAX}) CHECK(refused(k, 1, 6, taps.data(), 7));
    for (const Ratio q : kBadRatios) CHECK(refused(4, q.L, q.D, taps.data(), 7));
    CHECK(refused(4, 1, 6, taps.data(), 0));               // no taps, and not 1 / 1
    CHECK(refused(4, 2, 3, nullptr, 0));
    CHECK(refused(4, 1, 6, nullptr, 7));                   // NULL taps
    CHECK(refused(4, 1, 6, taps.data(), -1));
    CHECK(refused(4, 1, 6, taps.data(), RFA_AUDIO_RS_MAX_PHASE_TAPS + 1));      // J above 4096
    CHECK(refused(4, 2, 3, taps.data(), 2 * RFA_AUDIO_RS_MAX_PHASE_TAPS + 1));
    CHECK(refused(4, 147, 640, taps.data(), RFA_AUDIO_RS_MAX_TAPS + 1));        // T above 16384
    CHECK(refused(4, 1, 6, taps.data(), INT32_MAX));
    for (float bad : {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::nanf("")}) {
        float t3[3] = {1.0f, bad, 2.0f};
        CHECK(refused(4, 1, 6, t3, 3));
    }
    // valid requests: the device is looked for only now
    static const Shape ok[] = {{1, 1, 0}, {1, 6, 219}, {1, 2, 4096}, {147, 640, 16384}};
    for (const Shape q : ok)
        for (int32_t k : {1, RFA_AUDIO_RS_MAX_CHANNELS}) {
            s = reinterpret_cast<rfa_audio_rs *>(0x1);
            const int st = rfa_audio_rs_create(0, k, q.L, q.D, q.T ? taps.data() : nullptr, q.T, &s);
            CHECK(st == RFA_ERR_NODEVICE || st == RFA_OK);
            CHECK(st == RFA_OK || s == nullptr);
            if (st == RFA_OK && s) CHECK(rfa_audio_rs_destroy(s) == RFA_OK);
        }
}

static void check_null_handle() {
    CHECK(rfa_audio_rs_destroy(nullptr) == RFA_ERR_INVALID);
    CHECK(std::strcmp(rfa_audio_rs_last_error(nullptr), "null handle") == 0);
    int32_t v = 9, w = 9;
    size_t cnt[2] = {2, 2}, out[2] = {9, 9};
    float x[4] = {9.0f, 9.0f, 9.0f, 9.0f}, y[4] = {9.0f, 9.0f, 9.0f, 9.0f};
    int16_t q[4] = {9, 9, 9, 9};
    void *st = nullptr;
    CHECK(rfa_audio_rs_get_channels(nullptr, &v) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_get_ratio(nullptr, &v, &w) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_get_taps(nullptr, y, 4, &v) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_get_offset(nullptr, 0, &v) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_reset(nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_reset(nullptr, -1) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_process(nullptr, x, 2, cnt, y, 2, q, 2, out) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_process(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_process_host(nullptr, x, 2, cnt, y, 2, q, 2, out) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_set_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_get_stream(nullptr, &st) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_get_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_synchronize(nullptr) == RFA_ERR_INVALID);
    // nothing written through a null handle
    CHECK(v == 9 && w == 9 && y[0] == 9.0f && y[3] == 9.0f && q[0] == 9 && out[0] == 9 && out[1] == 9);
}

// With a device: the getters and the argument errors of a live handle.  Without one this part is
// skipped and says so; tests/test_gpu_audio_rs.py runs them on the device.
static void check_live() {
    rfa_audio_rs *s = nullptr;
    const float taps[5] = {0.1f, 0.2f, 0.4f, 0.2f, 0.1f};
    if (rfa_audio_rs_create(0, 2, 1, 3, taps, 5, &s) != RFA_OK) {
        std::printf("audio_rs_host_check: no device, live-handle checks (getters, argument errors) skipped\n");
        return;
    }
    int32_t v = 0, w = 0;
    CHECK(rfa_audio_rs_get_channels(s, &v) == RFA_OK && v == 2);
    CHECK(rfa_audio_rs_get_ratio(s, &v, &w) == RFA_OK && v == 1 && w == 3);
    CHECK(rfa_audio_rs_get_ratio(s, nullptr, &w) == RFA_ERR_INVALID);
    float got[8] = {};
    CHECK(rfa_audio_rs_get_taps(s, nullptr, 0, &v) == RFA_OK && v == 5);
    CHECK(rfa_audio_rs_get_taps(s, got, 8, &v) == RFA_OK && std::memcmp(got, taps, sizeof(taps)) == 0 && got[5] == 0.0f);
    CHECK(rfa_audio_rs_get_offset(s, 2, &v) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_get_offset(s, -1, &v) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_get_offset(s, 1, &v) == RFA_OK && v == 0);
    CHECK(rfa_audio_rs_reset(s, 2) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_reset(s, -2) == RFA_ERR_INVALID);
    float dummy[32] = {};                                  // never dereferenced: these calls fail their checks
    int16_t *pcm = reinterpret_cast<int16_t *>(dummy + 16);
    size_t cnt[2] = {6, 6}, zero[2] = {0, 0}, out[2] = {9, 9};
    CHECK(rfa_audio_rs_process(s, nullptr, 8, cnt, dummy + 16, 8, nullptr, 0, out) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_process(s, dummy, 8, cnt, nullptr, 0, nullptr, 0, out) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_process(s, dummy, 8, nullptr, dummy + 16, 8, nullptr, 0, out) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_process(s, dummy, 5, cnt, dummy + 16, 8, nullptr, 0, out) == RFA_ERR_INVALID);    // above in_stride
    CHECK(rfa_audio_rs_process(s, dummy, 8, cnt, dummy + 16, 1, nullptr, 0, out) == RFA_ERR_INVALID);    // above f32_stride
    CHECK(rfa_audio_rs_process(s, dummy, 8, cnt, nullptr, 0, pcm, 1, out) == RFA_ERR_INVALID);           // above s16_stride
    CHECK(rfa_audio_rs_process(s, dummy, 8, cnt, dummy, 8, nullptr, 0, out) == RFA_ERR_INVALID);         // in place
    CHECK(rfa_audio_rs_process(s, dummy, 8, cnt, nullptr, 0, reinterpret_cast<int16_t *>(dummy + 5), 16, out) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_process(s, dummy, 8, cnt, dummy + 16, 8, pcm + 1, 16, out) == RFA_ERR_INVALID);   // the outputs overlap
    CHECK(rfa_audio_rs_process(s, dummy, 8, cnt, nullptr, 0, reinterpret_cast<int16_t *>(reinterpret_cast<char *>(pcm) + 1), 8, out) == RFA_ERR_INVALID);
    CHECK(rfa_audio_rs_process(s, nullptr, 0, zero, nullptr, 0, nullptr, 0, out) == RFA_OK);             // no samples: nothing is looked at
    CHECK(out[0] == 0 && out[1] == 0);
    CHECK(rfa_audio_rs_process_host(s, nullptr, 0, zero, nullptr, 0, nullptr, 0, nullptr) == RFA_OK);
    CHECK(rfa_audio_rs_get_offset(s, 0, &v) == RFA_OK && v == 0);
    CHECK(rfa_audio_rs_destroy(s) == RFA_OK);
}

int main() {
    check_counts();
    check_plan();
    check_create_errors();
    check_null_handle();
    check_live();
    if (failures) {
        std::fprintf(stderr, "audio_rs_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("audio_rs_host_check ok\n");
    return 0;
}
