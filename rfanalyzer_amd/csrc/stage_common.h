// stage_common.h -- what the streaming stages (ddc.hip, demod.hip, channelizer.hip) and the slot
// meters (slot_sum.h) share.
//
// Host: the handle core (device, stream, last error) with the entries every stage exports in
// the same form -- set_stream / get_stream / synchronize / the stream's end in destroy -- the
// device check and stream creation of the create entries, the growth of a staging buffer, the
// checks and the upload of a bank call's planar rows and the choice of a kernel template by
// input format.
// Device: the one definition of the raw-sample conversion (IQConverter's lookup tables as
// arithmetic) and the unfused LDS pair load.  The channelizer is bit-exact against the front
// end because both convert through raw_to_iq below.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "../../include/rfa.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------- host

struct StageCore {
    int device = 0;
    hipStream_t stream = nullptr;       // where work is enqueued (own_stream or the caller's)
    hipStream_t own_stream = nullptr;   // created by the handle; set once *_set_stream is used
    std::string err;
};

template <class H>
int stage_fail(H *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    return code;
}

#define STAGE_HIP(h, expr)                                                             \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) return stage_fail((h), RFA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// Bytes of one complex input sample; 0 for a format the stages do not read.
inline size_t stage_sample_bytes(int fmt) {
    switch (fmt) {
    case RFA_IN_S8:
    case RFA_IN_U8: return 2;
    case RFA_IN_S16LE: return 4;
    case RFA_IN_F32_INTERLEAVED: return 8;
    default: return 0;
    }
}

// f(std::integral_constant<int, FMT>) for the handle's format (validated at creation).
template <class F>
auto stage_dispatch_format(int fmt, F &&f) {
    switch (fmt) {
    case RFA_IN_S8: return f(std::integral_constant<int, RFA_IN_S8>{});
    case RFA_IN_U8: return f(std::integral_constant<int, RFA_IN_U8>{});
    case RFA_IN_S16LE: return f(std::integral_constant<int, RFA_IN_S16LE>{});
    default: return f(std::integral_constant<int, RFA_IN_F32_INTERLEAVED>{});
    }
}

// A create entry checks its own arguments first, then the device.
inline int stage_check_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return RFA_ERR_NODEVICE;
    if (device < 0 || device >= count) return RFA_ERR_INVALID;
    return RFA_OK;
}

// The handle's own non-blocking stream on `device`.
template <class H>
int stage_open(H *h, int device) {
    h->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
        return RFA_ERR_HIP;
    return RFA_OK;
}

template <class H>
int stage_synchronize(H *h) {
    if (!h) return RFA_ERR_INVALID;
    STAGE_HIP(h, hipSetDevice(h->device));
    STAGE_HIP(h, hipStreamSynchronize(h->stream));
    return RFA_OK;
}

// What a stage carries between calls (history, tables, state) is ordered on the handle's
// stream: drain it before work moves to another one.
template <class H>
int stage_set_stream(H *h, void *stream) {
    const int rc = stage_synchronize(h);
    if (rc != RFA_OK) return rc;
    if (h->own_stream == nullptr) h->own_stream = h->stream;
    h->stream = stream ? (hipStream_t)stream : h->own_stream;
    return RFA_OK;
}

template <class H>
int stage_get_stream(const H *h, void **stream) {
    if (!h || !stream) return RFA_ERR_INVALID;
    *stream = (void *)h->stream;
    return RFA_OK;
}

template <class H>
const char *stage_last_error(const H *h) {
    return h ? h->err.c_str() : "null handle";
}

// First step of a destroy entry: drain the current stream and end the one the handle made.
template <class H>
void stage_close_stream(H *h) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    hipStream_t own = h->own_stream ? h->own_stream : h->stream;
    if (own) (void)hipStreamDestroy(own);
    h->stream = h->own_stream = nullptr;
}

// At least `want` elements behind p (bytes where p is a void *), nothing kept; small
// requests are rounded up to 4096 elements.  The stream is drained before the old buffer goes.
template <class H, class T>
int stage_grow(H *h, T *&p, size_t &cap, size_t want, const char *what) {
    if (want <= cap) return RFA_OK;
    STAGE_HIP(h, hipStreamSynchronize(h->stream));
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    want = std::max(want, (size_t)4096);
    if (hipMalloc(&p, want * sizeof(std::conditional_t<std::is_void_v<T>, char, T>)) != hipSuccess)
        return stage_fail(h, RFA_ERR_NOMEM, std::string("hipMalloc ") + what);
    cap = want;
    return RFA_OK;
}

// The planar input rows of a bank call: K rows of n_samples floats, channel_stride apart.
template <class H>
int stage_check_rows(H *h, size_t K, const float *re, const float *im, size_t channel_stride, size_t n_samples) {
    if (n_samples > (size_t)1 << 36 || channel_stride > (size_t)1 << 40)
        return stage_fail(h, RFA_ERR_INVALID, "n_samples too large");
    if (n_samples && (!re || !im)) return stage_fail(h, RFA_ERR_INVALID, "null input");
    if (K > 1 && channel_stride < n_samples) return stage_fail(h, RFA_ERR_INVALID, "channel_stride below n_samples");
    return RFA_OK;
}

// Such rows from host memory into the staging buffer d_in as [2][K][n_samples]: re rows, then im
// rows, on the handle's stream.
template <class H>
int stage_upload_rows(H *h, float *&d_in, size_t &cap, const float *re, const float *im, size_t channel_stride,
                      size_t K, size_t n_samples) {
    STAGE_HIP(h, hipSetDevice(h->device));
    const int rc = stage_grow(h, d_in, cap, 2 * K * n_samples, "input staging");
    if (rc != RFA_OK || n_samples == 0) return rc;
    const size_t row = n_samples * sizeof(float), pitch = (K > 1 ? channel_stride : n_samples) * sizeof(float);
    STAGE_HIP(h, hipMemcpy2DAsync(d_in, row, re, pitch, row, K, hipMemcpyHostToDevice, h->stream));
    STAGE_HIP(h, hipMemcpy2DAsync(d_in + K * n_samples, row, im, pitch, row, K, hipMemcpyHostToDevice, h->stream));
    return RFA_OK;
}

// ---------------------------------------------------------------- device

template <int FMT> struct RawOf { using type = unsigned; };
template <> struct RawOf<RFA_IN_F32_INTERLEAVED> { using type = float2; };

// Complex input sample g as stored (I,Q bytes / int16 pair / float pair).
template <int FMT>
__device__ __forceinline__ typename RawOf<FMT>::type raw_load(const void *raw, long long g) {
    if constexpr (FMT == RFA_IN_F32_INTERLEAVED) return static_cast<const float2 *>(raw)[g];
    else if constexpr (FMT == RFA_IN_S16LE) return static_cast<const unsigned *>(raw)[g];
    else return static_cast<const unsigned short *>(raw)[g];
}

// The reference's lookup-table conversion of one stored sample (source/Signed8BitIQConverter.java,
// Unsigned8BitIQConverter.java, Signed16BitIQConverter.kt), before any mixing.
template <int FMT>
__device__ __forceinline__ void raw_to_iq(typename RawOf<FMT>::type v, float &i, float &q) {
    if constexpr (FMT == RFA_IN_F32_INTERLEAVED) {
        i = v.x;
        q = v.y;
    } else if constexpr (FMT == RFA_IN_S16LE) {
        i = (float)(short)(v & 0xffffu) / 32768.0f;
        q = (float)(short)(v >> 16) / 32768.0f;
    } else if constexpr (FMT == RFA_IN_S8) {
        i = (float)(signed char)(v & 0xffu) / 128.0f;
        q = (float)(signed char)(v >> 8) / 128.0f;
    } else {
        i = ((float)(v & 0xffu) - 127.4f) / 128.0f;
        q = ((float)(v >> 8) - 127.4f) / 128.0f;
    }
}

typedef float v2f __attribute__((ext_vector_type(2)));

// One staged (re, im) pair as its own ds_read_b64.  A volatile LDS access keeps
// the compiler from fusing neighbours into ds_read2_b64, which moves half the
// bytes per LDS cycle on gfx950 (MI355X_MICROARCH.md, LDS table); the loads
// still issue back to back with counted waits (measured 3-9 % faster,
// profiles/r01o/ddc_unfused_lds_reads_ab.txt).
__device__ __forceinline__ v2f lds_ld(const v2f *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const volatile __attribute__((address_space(3))) v2f *)(p);
#else
    return *p;
#endif
}

__device__ __forceinline__ float2 lds_ld(const float2 *p) {
    const v2f v = lds_ld(reinterpret_cast<const v2f *>(p));
    return float2{v.x, v.y};
}
