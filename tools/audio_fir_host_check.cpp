// Host-side check of the audio FIR bank's C-ABI entries that need no device: rfa_audio_fir_plan,
// rfa_audio_fir_history_source (the kernel's own arithmetic for where a history sample comes from,
// walked across the boundary between the old history and the call's inputs), and every argument
// error of rfa_audio_fir_* that returns before any HIP call; with a device also the tap round
// trips at 0, 1 and 4096 taps and the argument errors of a live handle.
// Built together with rfanalyzer_amd/csrc/audio_fir.hip with the host compiled under
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

static const int H = RFA_AUDIO_FIR_MAX_TAPS - 1;
static const size_t kMaxCount = (size_t)1 << 36;

static void check_plan() {
    int32_t p[RFA_AUDIO_FIR_PLAN_FIELDS];
    const int32_t taps[] = {0, 1, 2, 3, 64, 65, 1309, RFA_AUDIO_FIR_MAX_TAPS};
    const size_t counts[] = {0, 1, 2, RFA_AUDIO_FIR_NARROW_MAX - 1, RFA_AUDIO_FIR_NARROW_MAX, RFA_AUDIO_FIR_NARROW_MAX + 1,
                             RFA_AUDIO_FIR_TILE - 1, RFA_AUDIO_FIR_TILE, RFA_AUDIO_FIR_TILE + 1, 2 * RFA_AUDIO_FIR_TILE + 17,
                             kMaxCount};
    for (int32_t T : taps)
        for (size_t n : counts) {
            for (int32_t &v : p) v = -9;
            CHECK(rfa_audio_fir_plan(T, n, p) == RFA_OK);
            CHECK(p[0] == RFA_AUDIO_FIR_TILE);
            const int path = n == 0 ? RFA_AUDIO_FIR_PATH_NONE
                             : T == 0 ? RFA_AUDIO_FIR_PATH_COPY
                             : n <= RFA_AUDIO_FIR_NARROW_MAX ? RFA_AUDIO_FIR_PATH_NARROW
                                                             : RFA_AUDIO_FIR_PATH_WIDE;
            CHECK(p[2] == path);
            CHECK(p[3] == (path == RFA_AUDIO_FIR_PATH_NARROW ? 2 : path == RFA_AUDIO_FIR_PATH_WIDE ? 8 : 0));
            CHECK((size_t)p[4] == (n + RFA_AUDIO_FIR_TILE - 1) / RFA_AUDIO_FIR_TILE);
            if (path == RFA_AUDIO_FIR_PATH_NARROW || path == RFA_AUDIO_FIR_PATH_WIDE) {
                // taps, then the tile's samples with T-1 before them, the alignment pad and the window's slack
                const size_t span = n < RFA_AUDIO_FIR_TILE ? n : RFA_AUDIO_FIR_TILE;
                CHECK(p[1] % 16 == 0);
                CHECK((size_t)p[1] >= sizeof(float) * ((size_t)T + span + (size_t)T - 1 + 3 + 9));
                CHECK(p[1] <= 64 * 1024);                  // the default dynamic LDS limit of a launch
                CHECK(p[3] * 256 >= (int)span);            // a thread's outputs cover the tile
            } else {
                CHECK(p[1] == 0);
            }
        }
    for (int32_t &v : p) v = -9;
    CHECK(rfa_audio_fir_plan(-1, 10, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_plan(RFA_AUDIO_FIR_MAX_TAPS + 1, 10, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_plan(INT32_MIN, 10, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_plan(INT32_MAX, 10, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_plan(5, kMaxCount + 1, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_plan(5, SIZE_MAX, p) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_plan(5, 10, nullptr) == RFA_ERR_INVALID);
    CHECK(p[0] == -9 && p[4] == -9);
}

// The history after a call is the last H samples of (history ++ inputs): sample j comes from
// position n + j of that row.
static void check_history_source() {
    const size_t counts[] = {0, 1, 2, (size_t)H - 1, (size_t)H, (size_t)H + 1, 2 * (size_t)H, 2 * (size_t)H + 1,
                             kMaxCount - 1, kMaxCount};
    for (size_t n : counts)
        for (int32_t j : {0, 1, H / 2, H - 2, H - 1}) {
            int32_t from = -9;
            size_t idx = 99;
            CHECK(rfa_audio_fir_history_source(n, j, &from, &idx) == RFA_OK);
            const size_t at = n + (size_t)j;
            CHECK(from == (at >= (size_t)H ? 1 : 0));
            CHECK(idx == (at >= (size_t)H ? at - (size_t)H : at));
            CHECK(from ? idx < n : idx < (size_t)H);        // inside the row it names
        }
    // every sample across the boundary for counts around it: old samples move down by n, the inputs follow
    for (size_t n : {(size_t)0, (size_t)1, (size_t)7, (size_t)H - 1, (size_t)H, (size_t)H + 5}) {
        size_t from_input = 0;
        for (int32_t j = 0; j < H; j++) {
            int32_t from = -9;
            size_t idx = 0;
            CHECK(rfa_audio_fir_history_source(n, j, &from, &idx) == RFA_OK);
            if (from) {
                CHECK(idx == n - (size_t)(H - j));         // the newest sample is the last input
                from_input++;
            } else {
                CHECK(idx == (size_t)j + n);
            }
        }
        CHECK(from_input == (n < (size_t)H ? n : (size_t)H));
    }
    int32_t from = -9;
    size_t idx = 99;
    CHECK(rfa_audio_fir_history_source(5, -1, &from, &idx) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_history_source(5, H, &from, &idx) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_history_source(5, INT32_MAX, &from, &idx) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_history_source(5, INT32_MIN, &from, &idx) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_history_source(kMaxCount + 1, 0, &from, &idx) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_history_source(SIZE_MAX, 0, &from, &idx) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_history_source(5, 0, nullptr, &idx) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_history_source(5, 0, &from, nullptr) == RFA_ERR_INVALID);
    CHECK(from == -9 && idx == 99);
}

static void check_create_errors() {
    rfa_audio_fir *f = reinterpret_cast<rfa_audio_fir *>(0x1);
    CHECK(rfa_audio_fir_create(0, 4, nullptr) == RFA_ERR_INVALID);
    for (int32_t k : {0, -1, RFA_AUDIO_FIR_MAX_CHANNELS + 1, INT32_MIN, INT32_MAX}) {
        f = reinterpret_cast<rfa_audio_fir *>(0x1);
        CHECK(rfa_audio_fir_create(0, k, &f) == RFA_ERR_INVALID && f == nullptr);
    }
    // valid requests: the device is looked for only now
    for (int32_t k : {1, 32, RFA_AUDIO_FIR_MAX_CHANNELS}) {
        f = reinterpret_cast<rfa_audio_fir *>(0x1);
        const int st = rfa_audio_fir_create(0, k, &f);
        CHECK(st == RFA_ERR_NODEVICE || st == RFA_OK);
        CHECK(st == RFA_OK || f == nullptr);
        if (st == RFA_OK && f) CHECK(rfa_audio_fir_destroy(f) == RFA_OK);
    }
}

static void check_null_handle() {
    CHECK(rfa_audio_fir_destroy(nullptr) == RFA_ERR_INVALID);
    CHECK(std::strcmp(rfa_audio_fir_last_error(nullptr), "null handle") == 0);
    int32_t w = 9;
    size_t cnt[2] = {2, 2};
    float x[4] = {9.0f, 9.0f, 9.0f, 9.0f}, y[4] = {9.0f, 9.0f, 9.0f, 9.0f};
    void *st = nullptr;
    CHECK(rfa_audio_fir_get_channels(nullptr, &w) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_get_channels(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_set_taps(nullptr, 0, x, 4) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_set_taps(nullptr, 0, nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_get_taps(nullptr, 0, y, 4, &w) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_reset(nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_reset(nullptr, -1) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_process(nullptr, x, 2, cnt, y, 2) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_process(nullptr, nullptr, 0, nullptr, nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_process_host(nullptr, x, 2, cnt, y, 2) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_process_host(nullptr, nullptr, 0, nullptr, nullptr, 0) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_set_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_get_stream(nullptr, &st) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_get_stream(nullptr, nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_synchronize(nullptr) == RFA_ERR_INVALID);
    // nothing written through a null handle
    CHECK(w == 9 && y[0] == 9.0f && y[3] == 9.0f && x[0] == 9.0f);
}

// With a device: tap round trips and the argument errors of a live handle.  A handle needs device
// memory; without one this part is skipped and says so.
static void check_live() {
    rfa_audio_fir *f = nullptr;
    if (rfa_audio_fir_create(0, 2, &f) != RFA_OK) {
        std::printf("audio_fir_host_check: no device, live-handle checks (tap round trips, argument errors) skipped\n");
        return;
    }
    int32_t w = 0;
    CHECK(rfa_audio_fir_get_channels(f, &w) == RFA_OK && w == 2);
    CHECK(rfa_audio_fir_get_channels(f, nullptr) == RFA_ERR_INVALID);
    std::vector<float> taps(RFA_AUDIO_FIR_MAX_TAPS + 1), got(RFA_AUDIO_FIR_MAX_TAPS, -1.0f);
    for (size_t j = 0; j < taps.size(); j++) taps[j] = 1.0f / (float)(j + 1);
    for (int32_t T : {0, 1, RFA_AUDIO_FIR_MAX_TAPS, 1, 0}) {
        CHECK(rfa_audio_fir_set_taps(f, 1, taps.data(), T) == RFA_OK);
        int32_t n = -1;
        CHECK(rfa_audio_fir_get_taps(f, 1, nullptr, 0, &n) == RFA_OK && n == T);
        std::fill(got.begin(), got.end(), -1.0f);
        CHECK(rfa_audio_fir_get_taps(f, 1, got.data(), got.size(), &n) == RFA_OK && n == T);
        CHECK(std::memcmp(got.data(), taps.data(), (size_t)T * sizeof(float)) == 0);
        CHECK(T == RFA_AUDIO_FIR_MAX_TAPS || got[(size_t)T] == -1.0f);
        CHECK(rfa_audio_fir_get_taps(f, 0, nullptr, 0, &n) == RFA_OK && n == 0);     // the other slot is untouched
    }
    CHECK(rfa_audio_fir_set_taps(f, 0, nullptr, 0) == RFA_OK);
    CHECK(rfa_audio_fir_set_taps(f, 0, nullptr, 3) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_set_taps(f, 2, taps.data(), 3) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_set_taps(f, -1, taps.data(), 3) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_set_taps(f, 0, taps.data(), -1) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_set_taps(f, 0, taps.data(), RFA_AUDIO_FIR_MAX_TAPS + 1) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_set_taps(f, 0, taps.data(), 3) == RFA_OK);
    for (float bad : {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::nanf("")}) {
        float t3[3] = {1.0f, bad, 2.0f};
        int32_t n = -1;
        CHECK(rfa_audio_fir_set_taps(f, 0, t3, 3) == RFA_ERR_INVALID);
        CHECK(rfa_audio_fir_get_taps(f, 0, got.data(), got.size(), &n) == RFA_OK && n == 3 && got[1] == taps[1]);
    }
    int32_t n = 0;
    CHECK(rfa_audio_fir_get_taps(f, 2, got.data(), got.size(), &n) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_get_taps(f, 0, got.data(), got.size(), nullptr) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_reset(f, 2) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_reset(f, -2) == RFA_ERR_INVALID);
    float *x = nullptr;                                    // never dereferenced: these calls fail their checks
    float dummy[16] = {};
    size_t cnt[2] = {2, 2}, zero[2] = {0, 0};
    CHECK(rfa_audio_fir_process(f, nullptr, 4, cnt, dummy, 4) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_process(f, dummy, 4, cnt, x, 4) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_process(f, dummy, 4, nullptr, dummy + 8, 4) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_process(f, dummy, 1, cnt, dummy + 8, 4) == RFA_ERR_INVALID);     // a count above in_stride
    CHECK(rfa_audio_fir_process(f, dummy, 4, cnt, dummy + 8, 1) == RFA_ERR_INVALID);     // ... above out_stride
    CHECK(rfa_audio_fir_process(f, dummy, 4, cnt, dummy, 4) == RFA_ERR_INVALID);         // in place
    CHECK(rfa_audio_fir_process(f, dummy, 4, cnt, dummy + 1, 4) == RFA_ERR_INVALID);     // overlapping
    CHECK(rfa_audio_fir_process(f, dummy, 4, cnt, dummy + 5, 4) == RFA_ERR_INVALID);     // row 1 of in, row 0 of out
    cnt[1] = kMaxCount + 1;
    CHECK(rfa_audio_fir_process(f, dummy, (size_t)1 << 37, cnt, dummy + 8, (size_t)1 << 37) == RFA_ERR_INVALID);
    CHECK(rfa_audio_fir_process(f, nullptr, 0, zero, nullptr, 0) == RFA_OK);             // no samples: nothing is looked at
    CHECK(rfa_audio_fir_process_host(f, nullptr, 0, zero, nullptr, 0) == RFA_OK);
    CHECK(rfa_audio_fir_destroy(f) == RFA_OK);
}

int main() {
    check_plan();
    check_history_source();
    check_create_errors();
    check_null_handle();
    check_live();
    if (failures) {
        std::fprintf(stderr, "audio_fir_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("audio_fir_host_check ok\n");
    return 0;
}
