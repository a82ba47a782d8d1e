/*
 * rfa.h -- C-ABI of the MI355X-native RFAnalyzer spectrum pipeline (librfa.so).
 *
 * Replaces the reference's spectrum hot path (thomasjoergensen/RFAnalyzer):
 *
 *   reference interface                                   replaced by
 *   ----------------------------------------------------  -------------------------------------
 *   NativeDsp.performWindowedFftAndReturnMag(re,im,mag)    rfa_windowed_fft_mag_planar()
 *     nativedsp/src/main/java/com/mantz_it/nativedsp/NativeDsp.kt:43-62
 *   JNI performFFTAndLogMag(in[2N], out[N])                rfa_fft_logmag_interleaved()
 *     nativedsp/src/main/cpp/nativedsp.cpp:44-81
 *   JNI performFFT(in[2N], out[2N])                        rfa_fft_ordered()
 *     nativedsp/src/main/cpp/nativedsp.cpp:19-42
 *   IQConverter.fillPacketIntoSamplePacket + window + FFT  rfa_process() / rfa_process_host()
 *     source/Signed8BitIQConverter.java:80-99,                (raw IQ bytes in, fused on device)
 *     Unsigned8BitIQConverter.java:80-99,
 *     Signed16BitIQConverter.kt:89-124, Scheduler.kt:252-279
 *   FftProcessor.run ring write / retune shift / peak-hold rfa_process(), rfa_set_tuning(),
 *     analyzer/FftProcessor.kt:164-245                        rfa_get_ring(), rfa_get_peaks()
 *   AnalyzerSurface boxcar time average                    rfa_get_boxcar()
 *     ui/AnalyzerSurface.kt:657-714
 *   AnalyzerSurface.drawPreprocessing (colour rows, path)  rfa_draw_preprocess()
 *     ui/AnalyzerSurface.kt:599-743
 *   MainViewModel scanner / squelch row reductions          rfa_row_window_stats()
 *     ui/MainViewModel.kt:861-929,1391-1540
 *   the same reductions for every frame of a batch         rfa_set_windows(), rfa_get_window_stats(),
 *     ui/MainViewModel.kt:861-929,1151-1250,1392-1550        rfa_ring_window_stats()
 *   IQConverter.mixPacketIntoSamplePacket + Decimator      rfa_ddc_*() (demod front end, below)
 *     source/Signed8BitIQConverter.java:53-131, analyzer/Decimator.java:175-191
 *   Resampler / RationalResampler (live demod path)        rfa_ddc_create_resampler()
 *     analyzer/Resampler.kt:102-110, dsp/RationalResampler.kt:27-127
 *   the two above for K channels of one raw packet         rfa_ddc_bank_*() (channel bank, below)
 *   K Demodulators with their AudioSinks, one set of launches rfa_demod_bank_*() (demodulator bank, below)
 *   Scheduler's per-packet squelch gate, per bank slot     rfa_squelch_*() (squelch bank, below)
 *     analyzer/Scheduler.kt:52,161-165,237, database/AppStateRepository.kt:318-324
 *   (extension) every channel of a uniform raster per call rfa_pfb_*() (polyphase channelizer, below;
 *     rfa_pfb_create_rational: at any source sample rate)
 *   (extension) frequency error of every bank slot         rfa_freq_*() (frequency meter bank, below)
 *   (extension) CTCSS tone sums of every bank slot's audio rfa_tone_*() (tone meter bank, below)
 *   (extension) DCS sub-cell sums of every bank slot's audio rfa_code_*() (code meter bank, below)
 *   (extension) a real FIR on every bank slot's audio      rfa_audio_fir_*() (audio FIR bank, below)
 *   (extension) every bank slot's audio to 8 / 16 kHz PCM  rfa_audio_rs_*() (audio resampler bank, below)
 *   (extension) recursive sections on every slot's audio   rfa_audio_iir_*() (audio IIR bank, below)
 *   (north-star extension) exponential average             rfa_get_ema()
 *     idiom of database/GlobalPerformanceData.kt:44-50
 *
 * (app paths are relative to app/src/main/java/com/mantz_it/rfanalyzer/.)
 *
 * Conventions
 *  - Every function returns an int status: RFA_OK (0) or a negative RFA_ERR_*.
 *  - A handle is single-threaded; separate handles are independent (one per
 *    GPU / HIP stream).  There is no process-global state.
 *  - Output rows are 10*log10(|X_k|/N) (nativedsp.cpp:78), fft-shifted so that
 *    out[t] holds bin (t + N/2) mod N (out[0] = -fs/2, out[N/2] = DC).
 *  - N is a power of two, RFA_MIN_FFT_SIZE..RFA_MAX_FFT_SIZE.
 *  - Device pointers are HIP device (or host-coherent) addresses; work is
 *    enqueued on the handle's stream and is asynchronous unless the function
 *    name ends in _host or the doc says it synchronises.
 */
#ifndef RFA_H
#define RFA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef RFA_API
#define RFA_API __attribute__((visibility("default")))
#endif

#define RFA_ABI_VERSION 1
#define RFA_MIN_FFT_SIZE 64
#define RFA_MAX_FFT_SIZE (1 << 20)

enum rfa_status {
    RFA_OK = 0,
    RFA_ERR_INVALID = -1,     /* NULL handle/pointer, bad enum, bad size  */
    RFA_ERR_SIZE = -2,        /* array length mismatch (NativeDsp.kt:45-46) */
    RFA_ERR_UNSUPPORTED = -3, /* fft size / mode not supported             */
    RFA_ERR_NODEVICE = -4,    /* no HIP device visible                     */
    RFA_ERR_NOMEM = -5,       /* device / host allocation failed           */
    RFA_ERR_HIP = -6,         /* HIP runtime error (see rfa_last_error)    */
    RFA_ERR_STATE = -7        /* operation needs a feature not enabled     */
};

enum rfa_window { RFA_WINDOW_BLACKMAN = 0, RFA_WINDOW_HANN = 1, RFA_WINDOW_NONE = 2 };

/* Raw IQ sample formats (IQ_FILE_FORMAT.md / the converters above). */
enum rfa_input_format {
    RFA_IN_S8 = 0,             /* HackRF: int8 I,Q        -> b/128            */
    RFA_IN_U8 = 1,             /* RTL-SDR: uint8 I,Q      -> (b-127.4f)/128   */
    RFA_IN_S16LE = 2,          /* Airspy/HydraSDR: int16  -> s/32768          */
    RFA_IN_F32_INTERLEAVED = 3,/* float I,Q                                   */
    RFA_IN_F32_PLANAR = 4      /* per frame: float re[N] then float im[N]     */
};

enum rfa_avg_mode { RFA_AVG_NONE = 0, RFA_AVG_BOXCAR = 1, RFA_AVG_EMA = 2 };

typedef struct rfa_config {
    int32_t fft_size;      /* N, power of two                                       */
    int32_t window;        /* enum rfa_window                                       */
    int32_t input_format;  /* enum rfa_input_format                                 */
    int32_t avg_mode;      /* enum rfa_avg_mode (boxcar reads the ring)             */
    int32_t avg_length;    /* boxcar: L (average of the newest L+1 rows), 0..ring   */
    float ema_alpha;       /* EMA: avg += alpha*(x-avg), 0 < alpha <= 1             */
    int32_t peak_hold;     /* 0/1 (FftProcessor.kt:229-245)                         */
    int32_t ring_rows;     /* waterfall rows R (500/400/300, FftProcessor.kt:103), 0 = no ring */
    int32_t device_id;     /* HIP device ordinal                                    */
} rfa_config;

typedef struct rfa_handle rfa_handle;

/* Library / device queries (no handle). */
RFA_API int rfa_abi_version(void);
RFA_API int rfa_device_count(int *count);
RFA_API const char *rfa_status_string(int status);
RFA_API void rfa_default_config(rfa_config *cfg); /* N=16384, Blackman, s8, no avg, no peak, 400 rows, dev 0 */

/* Lifetime. */
RFA_API int rfa_create(const rfa_config *cfg, rfa_handle **out);
RFA_API int rfa_destroy(rfa_handle *h);
RFA_API int rfa_get_config(const rfa_handle *h, rfa_config *cfg);
RFA_API const char *rfa_last_error(const rfa_handle *h);

/* Stream control: work is enqueued on exactly `stream` (a hipStream_t; NULL is
 * the HIP null stream) until rfa_use_own_stream() restores the handle's own
 * non-blocking stream. */
RFA_API int rfa_set_stream(rfa_handle *h, void *stream);
RFA_API int rfa_use_own_stream(rfa_handle *h);
RFA_API int rfa_get_stream(const rfa_handle *h, void **stream);
RFA_API int rfa_synchronize(rfa_handle *h);

/* Pipelined state (opt-in, no reference counterpart: FftProcessor.kt:135-245 runs the FFT,
 * the ring write and the peak-hold one after another on one thread).  state_cus > 0 reserves
 * that many CUs (a multiple of the device's XCD count, spread one per shader engine) for a
 * CU-masked state stream that runs each call's peak / EMA / channel-mean pass, while the
 * FFT kernels run on two CU-masked streams over the other CUs, alternating per call.  Call
 * k's state pass then runs under call k + 1's FFT: a call that rewrites the whole ring
 * (n_frames == ring_rows) writes the second ring buffer (the ring and its shift buffer swap
 * per call, so rfa_get_state_generation advances), a call of at most ring_rows / 2 frames
 * writes rows call k's pass does not read, and any other call waits for the previous pass.
 * Pipelined calls are those with rows == NULL, a ring holding the batch, and peak-hold or
 * EMA on; the rest run as before.
 * The handle stream is NOT ordered after a pipelined call: rfa_join(h) enqueues on it a wait
 * for every pipelined kernel so far (the input buffers may be reused and the ring / peaks /
 * EMA read on that stream after it); rfa_synchronize and every other entry point join first.
 * state_cus = 0 turns the mode off (after a join).  RFA_ERR_UNSUPPORTED when the device does
 * not take CU masks or state_cus leaves no CUs for the FFT. */
RFA_API int rfa_set_pipelined(rfa_handle *h, int32_t state_cus);
RFA_API int rfa_join(rfa_handle *h);

/* Batch processing.  `in` holds n_frames frames of N samples in the configured
 * format, frame f starting at byte f*frame_stride_bytes (0 = densely packed).
 * For a headerless file replayed in packets of P bytes with N <= P/bps, the
 * reference's framing (Scheduler.kt:252-279: each packet fills one frame,
 * the rest of the packet is dropped) is frame_stride_bytes = P.
 * Rows go to `rows` (n_frames*N floats, frame order; may be NULL) and, if
 * ring_rows > 0, into the device waterfall ring in the reference's reverse
 * order (frames of this batch that the reference would overwrite within the
 * same batch are not stored).  Peak-hold / EMA state advance frame by frame.
 *   rfa_process      : device pointers, asynchronous on the handle stream.
 *   rfa_process_host : host pointers; copies in/out and synchronises. */
RFA_API int rfa_process(rfa_handle *h, const void *in, size_t n_frames, size_t frame_stride_bytes, float *rows);
RFA_API int rfa_process_host(rfa_handle *h, const void *in, size_t n_frames, size_t frame_stride_bytes, float *rows);

/* Multi-batch enqueue: the result of n_batches consecutive rfa_process calls (ring,
 * peaks, EMA and channel means advance batch after batch; ring rows, peaks and
 * channel means identical, the EMA equal to fp32 rounding -- the packed launch's
 * chunked scan associates the recursion differently), batch b reading
 * frames_per_batch frames at in + b * batch_stride_bytes + f * frame_stride_bytes
 * and writing its rows (if rows != NULL) at rows + b * frames_per_batch * N.
 * When the batches are packed (batch_stride_bytes == frames_per_batch * frame
 * stride) the whole run is ONE kernel launch, so small batches (BASELINE
 * config 4: 256 x 8192 points) stop paying a host call + launch each.
 * Device pointers, asynchronous on the handle stream; rfa_get_channel_means then
 * returns the last batch's frames_per_batch means, in either form. */
RFA_API int rfa_process_batches(rfa_handle *h, const void *in, size_t n_batches, size_t batch_stride_bytes,
                                size_t frames_per_batch, size_t frame_stride_bytes, float *rows);

/* Scheduler.run's FFT branch, one raw packet at a time (Scheduler.kt:252-273
 * with the converters' fillPacketIntoSamplePacket, Signed8BitIQConverter.java:80-98,
 * Unsigned8BitIQConverter.java:80-98, Signed16BitIQConverter.kt:89-124): the
 * packet's whole samples (host bytes in the handle's input format) fill the
 * handle's partial frame from the packet start at startIndex = samples already
 * held; once it holds N samples the frame is processed like rfa_process_host
 * (ring, peaks, EMA, channel mean) after rfa_set_tuning(frequency, sample_rate)
 * of the packet that completed it, and the rest of that packet is dropped.  So
 * P-sample packets give one frame per packet when P >= N and one frame every
 * ceil(N / P) packets when P < N (e.g. RTL-SDR's 16 KiB = 8192-sample packets,
 * RtlsdrSource.java:112, at the default N = 16384).  *frames = 1 when a frame
 * was processed (its row copied to row_out, N floats, unless NULL), else 0.
 * Only the completing packet's frequency / sample_rate are used, so only its
 * sample_rate must be > 0 (else RFA_ERR_INVALID and the frame is dropped); a
 * packet that only partly fills the frame is always accepted.
 * Synchronous.  RFA_ERR_UNSUPPORTED for RFA_IN_F32_PLANAR.  rfa_reset_state and
 * rfa_set_fft_size discard a partial frame (Scheduler.kt:259-260);
 * rfa_pending_samples reports how many samples it holds. */
RFA_API int rfa_push_packet(rfa_handle *h, const void *packet, size_t packet_bytes, int64_t frequency,
                            int64_t sample_rate, float *row_out, int32_t *frames);
RFA_API int rfa_pending_samples(const rfa_handle *h, int64_t *samples);

/* Tuning metadata of the following frames (SamplePacket.frequency/sampleRate).
 * Mirrors FftProcessor.kt:169-220,238-239: a frequency change shifts every ring
 * row by (int)((f_old-f_new)*(N/(float)sr)) bins with -9999 fill (or clears it
 * when |shift| >= N); a sample-rate change clears the ring; either resets the
 * peaks and the EMA.  The first call only records the values (the ring starts
 * cleared). */
RFA_API int rfa_set_tuning(rfa_handle *h, int64_t frequency, int64_t sample_rate);

/* State read-back (synchronise the handle stream; host destination).
 * rfa_get_ring copies ring_rows*N floats in storage order and returns the
 * reference's readIndex (newest row) and writeIndex (FftProcessorData). */
RFA_API int rfa_get_peaks(rfa_handle *h, float *out);
RFA_API int rfa_get_ema(rfa_handle *h, float *out);
RFA_API int rfa_get_boxcar(rfa_handle *h, int32_t length, float *out);
RFA_API int rfa_get_ring(rfa_handle *h, float *out, int32_t *read_index, int32_t *write_index);
RFA_API int rfa_reset_state(rfa_handle *h); /* ring -> -9999, peaks/EMA -> uninitialised */

/* Waterfall speed change (FftProcessor.kt:185-195, waterfallSpeed -> 500/400/300
 * rows, :103).  As in the reference the ring is rebuilt when the next frame
 * arrives (inside rfa_process), keeping the history: new row i = old row
 * (writeIndex + i) % old_rows for i < old_rows, -9999 rows beyond, then
 * writeIndex = 0.  Until then the old ring, readIndex and writeIndex stay
 * valid.  ring_rows >= 1; RFA_ERR_INVALID when a boxcar average_length would
 * not fit.  A ring_rows == 0 handle gains a cleared ring. */
RFA_API int rfa_set_ring_rows(rfa_handle *h, int32_t ring_rows);
/* FFT size change (FftProcessor.kt:178-183 ring re-created at -9999 with
 * writeIndex = 0, :233-236 peaks re-initialised; the EMA restarts): every
 * per-N table and state buffer is rebuilt for fft_size; tuning, channel range,
 * stream and ring_rows carry over; the window list of rfa_set_windows is cleared (bin indices
 * do not survive a size change).  Synchronises. */
RFA_API int rfa_set_fft_size(rfa_handle *h, int32_t fft_size);

/* Channel signal strength for the squelch (FftProcessor.kt:143-157): for every
 * frame of each rfa_process batch, the mean dB over bins
 * [((start - f0) * (N / sampleRate.toFloat())).toInt(), same for end), each
 * clamped to [0, N], f0 = frequency - sampleRate / 2 (the tuning of
 * rfa_set_tuning).  start_frequency == end_frequency disables it.  The sum is a
 * deterministic parallel reduction: equal to the reference's sequential fp32 loop
 * (:150-152) over the same row to the rounding of the sum -- so a
 * frame whose mean lies within that rounding of the squelch threshold can fall on
 * the other side of it than in the reference.
 * rfa_get_channel_means copies the last batch's means in frame order
 * (synchronises); *count = 0 when the channel range is empty. */
RFA_API int rfa_set_channel(rfa_handle *h, int64_t start_frequency, int64_t end_frequency);
RFA_API int rfa_get_channel_means(rfa_handle *h, float *out, size_t capacity, size_t *count);

/* Display preprocessing: the reference's
 * AnalyzerSurface.drawPreprocessing (app/.../ui/AnalyzerSurface.kt:599-743)
 * computed on the device from the ring, for the tuning of rfa_set_tuning and the
 * newest row rfa_get_ring reports.  The handle keeps the draw thread's state:
 * a persistent colour buffer and the dirty map (waterfallBufferDirtyMap).  Rows
 * written by rfa_process are dirty; a retune, clear, ring resize, new width or
 * new viewport / vertical scale marks every row.  A draw refreshes, newest
 * first, every dirty row and rows 0..average_length, at most
 * average_length + 6 rows (AnalyzerSurface.kt:619-640,678-684); the other rows
 * keep their colours, exactly as in the reference.  Outputs (host, synchronous):
 *   colors      [ring_rows][width] ARGB, ring storage order (colorBuffer[bufferIndex*width + i]):
 *               colormap[clamp(((avg - min_db) * scale).toInt())] of the pixel's mean
 *               bin value, black (0xff000000) outside the drawn range;
 *   fft_path_y  [width]: fftHeight - (timeAverage - min_db) * dbWidth of the boxcar over
 *               the newest average_length + 1 rows (the fftPath points), NaN where the
 *               reference adds no point;
 *   peaks_y     [width] or NULL: peaksYCoordinates (-1 outside), needs peak_hold;
 *   autoscale   [2] or NULL: min / max of the time averages, starting from
 *               (10, -100) = (VERTICAL_SCALE_UPPER_BOUNDARY, _LOWER_BOUNDARY), before
 *               the reference's +-5 dB margin (AnalyzerSurface.kt:731-735).
 * Bit-identical to the JVM's fp32 arithmetic; where the reference would index the
 * row out of bounds (and throw) the bin is skipped. */
typedef struct rfa_draw_params {
    int32_t width;                /* surface width in pixels                           */
    int32_t fft_height;           /* spectrum plot height in pixels                    */
    int64_t viewport_frequency;   /* viewport centre frequency (Hz)                    */
    int64_t viewport_sample_rate; /* viewport span (Hz)                                */
    float min_db, max_db;         /* vertical scale (viewportVerticalScaleMin/Max)     */
    int32_t average_length;       /* fftAverageLength, < ring_rows                     */
    int32_t colormap_size;        /* entries of colormap                               */
    const uint32_t *colormap;     /* ARGB colours, e.g. ColorMaps.kt createGqrxMap()   */
} rfa_draw_params;
RFA_API int rfa_draw_preprocess(rfa_handle *h, const rfa_draw_params *p, uint32_t *colors, float *fft_path_y,
                                float *peaks_y, float *autoscale);

/* Scanner / squelch reductions of the newest ring row:
 * for each inclusive bin window [lo[i], hi[i]] of the fft-shifted newest row
 * (FftProcessorData.readIndex), peak = FloatArray.maxOrNull() (NaN wins) and
 * avg = FloatArray.average().toFloat() (double sum / count).  Replaces the JVM
 * loops of MainViewModel.kt:861-929 (detectIEMChannelsInFFT, window
 * +-max(5, (100000 / resolution).toInt()) bins), :1391-1457 (getAverageSignalLevel,
 * detectSignal: the whole row [0, N-1]) and :1462-1540 (detectSignalsInFFT,
 * +-2 bins per step); the window arithmetic and thresholds stay with the caller
 * (rfanalyzer_amd/scanner.py mirrors them).  Synchronous, host arrays. */
RFA_API int rfa_row_window_stats(rfa_handle *h, const int32_t *lo, const int32_t *hi, size_t count, float *peak,
                                 float *avg);

/* The same reductions for EVERY frame of a batch (no reference counterpart as a batch: the
 * reference's consumers reduce one row at a time -- detectSignalsInFFT MainViewModel.kt:1463-1550,
 * detectIEMChannelsInFFT :861-929, detectSignal / getAverageSignalLevel :1392-1457, the AirComm
 * pair :1151-1250 -- and a 500-frame rfa_process leaves them 500 rows).
 * rfa_set_windows keeps a list of inclusive windows [lo[i], hi[i]] over fft-shifted bins on the
 * handle (copied to the device; validated like rfa_row_window_stats: 0 <= lo <= hi <= N - 1, else
 * RFA_ERR_INVALID and the previous list stays).  count == 0 switches the feature off.  While a
 * list is set, every rfa_process / rfa_process_host / rfa_process_batches (and rfa_push_packet)
 * call also computes, for every frame f of the call and window i, peak[f][i] =
 * FloatArray.maxOrNull() (NaN wins) and avg[f][i] = FloatArray.average().toFloat() (double sum /
 * count, rounded once) -- what rfa_row_window_stats gives for that frame when it is the newest
 * row (peaks identical; averages equal up to the order of the double additions, one float ulp).
 * The work is asynchronous on the stream of the channel mean (the state stream in pipelined
 * mode), a bounded number of launches whatever the frame and window counts, and reads the rows
 * where the state pass reads them (caller rows, the ring when the batch fits, else a staging
 * buffer; the ring's storage order, reverse row order and wrap are handled inside).  A value
 * depends on its row and its window alone: the same for any split of a frame stream into calls,
 * any row source and any other windows in the list.  The list survives retunes, resets and ring
 * resizes; rfa_set_fft_size to another size clears it, because bin indices do not survive a size
 * change.  At least 65536 windows are accepted.
 * rfa_get_window_stats copies the last call's matrices, [frames][windows] in frame order and
 * the caller's window order (at most capacity_frames frames; *frames and *windows report the
 * full shape, 0 frames when no list is set or no call followed it), and synchronises; after
 * rfa_process_batches it is the last batch, as for rfa_get_channel_means.
 * rfa_get_window_stats_device returns the device matrices instead (after a join; valid until
 * the next process call, rfa_set_windows or a size change; NULL when *frames is 0).
 * rfa_ring_window_stats is the post-hoc form through the same kernel: the newest rows_back rows
 * of the ring (1 <= rows_back <= ring_rows), newest first, peak / avg [rows_back][count] host
 * arrays, synchronous; it leaves the handle's own list alone.  rows_back == 1 gives
 * rfa_row_window_stats' peaks bit for bit. */
RFA_API int rfa_set_windows(rfa_handle *h, const int32_t *lo, const int32_t *hi, size_t count);
RFA_API int rfa_get_window_stats(rfa_handle *h, float *peak, float *avg, size_t capacity_frames, size_t *frames,
                                 size_t *windows);
RFA_API int rfa_get_window_stats_device(rfa_handle *h, const float **peak, const float **avg, size_t *frames,
                                        size_t *windows);
RFA_API int rfa_ring_window_stats(rfa_handle *h, const int32_t *lo, const int32_t *hi, size_t count, int32_t rows_back,
                                  float *peak, float *avg);

/* Device-side state pointers, for zero-copy consumers.  peaks and EMA are in
 * natural (fft-shifted) bin order.  The ring's rows are stored in the order
 * rfa_get_ring_order reports.  The pointers (and the ring order) stay valid only
 * while rfa_get_state_generation returns the same value: a retune that shifts
 * the ring (rfa_set_tuning swaps the ring with its shift buffer), a ring resize
 * applied by rfa_process (rfa_set_ring_rows) and rfa_set_fft_size (which rebuilds
 * every buffer and frees the old ones) each advance it; re-query after a change. */
RFA_API int rfa_get_device_state(rfa_handle *h, float **ring, float **peaks, float **ema);
RFA_API int rfa_get_state_generation(const rfa_handle *h, int64_t *generation);

/* Storage order of the device ring rows (no reference counterpart: the JVM
 * waterfallBuffer rows are natural order, FftProcessor.kt:222-227, and
 * rfa_get_ring returns them so).  *residues = RS: the fft-shifted bin t of a
 * device ring row lives in block t mod RS of N/RS elements.  RS = 1 is one block;
 * the N = 64 K / 128 K kernels compute a frame as RS residue sub-FFTs and store
 * each residue's bins as one block (whole cache lines per workgroup); N = 256 K ..
 * 1 M use RS = N / 32768 (the large-N kernel B writes the bins S q + s of column
 * s as block s).  Inside a block, N = 32 K .. 128 K keep the 32 K-point kernel's
 * store tiles (16-B stores per lane); N = 256 K .. 1 M and N <= 16 K natural
 * order (bin t at block offset t / RS).  rfa_get_ring_positions fills the
 * storage position of every fft-shifted bin (positions[N]) for zero-copy
 * consumers; every rfa_* consumer of the ring handles the order internally. */
RFA_API int rfa_get_ring_order(const rfa_handle *h, int32_t *residues);
RFA_API int rfa_get_ring_positions(const rfa_handle *h, int32_t *positions, size_t count);

/* Reference-seam entry points (host arrays, synchronous).  They use the
 * handle's N; the window/format of the handle are ignored where the reference
 * symbol fixes them. */
/* NativeDsp.kt:43-62: Blackman-windowed FFT of planar re/im, log-mag row out.
 * Returns RFA_ERR_SIZE on length mismatch (the Kotlin method returns false). */
RFA_API int rfa_windowed_fft_mag_planar(rfa_handle *h, const float *re, const float *im, float *mag_out, size_t n);
/* nativedsp.cpp:44-81: already-windowed interleaved input (2N floats) -> N dB. */
RFA_API int rfa_fft_logmag_interleaved(rfa_handle *h, const float *in, float *mag_out, size_t n);
/* nativedsp.cpp:19-42: ordered, unscaled, forward complex FFT, 2N floats each. */
RFA_API int rfa_fft_ordered(rfa_handle *h, const float *in, float *out, size_t n);

/* The same three seams at every length the reference's pffft accepts
 * (pffft_new_setup, pffft.c:1231-1280: N a multiple of 16, N / 4 a product of
 * 2, 3, 4 and 5, N <= 2^26), one plan per N like nativedsp.cpp:12-17's cached
 * setup.  rfa_create covers the powers of two 64 .. 2^20 with its fused kernels;
 * a plan serves the rest (16, 32, 2^21 .. 2^26, mixed lengths such as 48 or
 * 3 * 2^20) with a mixed-radix Stockham FFT on the GPU (csrc/fft_seam.hip).
 * rfa_seam_create returns RFA_ERR_UNSUPPORTED for a length pffft rejects.
 * Synchronous, host arrays, RFA_ERR_SIZE on a length mismatch. */
typedef struct rfa_seam rfa_seam;
RFA_API int rfa_seam_supported(int32_t n); /* 1 when pffft accepts N, else 0 */
RFA_API int rfa_seam_create(int32_t n, int32_t device_id, rfa_seam **out);
RFA_API int rfa_seam_destroy(rfa_seam *s);
RFA_API const char *rfa_seam_last_error(const rfa_seam *s);
/* the pass radices (8, 4, 2, 3, 5), first pass first; count = number of passes */
RFA_API int rfa_seam_get_plan(const rfa_seam *s, int32_t *radices, int32_t cap, int32_t *count);
RFA_API int rfa_seam_windowed_fft_mag_planar(rfa_seam *s, const float *re, const float *im, float *mag_out, size_t n);
RFA_API int rfa_seam_fft_logmag_interleaved(rfa_seam *s, const float *in, float *mag_out, size_t n);
RFA_API int rfa_seam_fft_ordered(rfa_seam *s, const float *in, float *out, size_t n);

/* Profiling: while enabled, HIP events bracket every main FFT kernel launch on
 * the handle stream; rfa_get_kernel_time waits for and sums them.  Toggling
 * never synchronises, so a caller may profile a sample of its launches. */
/* Measurement support (no reference counterpart).  rfa_stream_copy: the device
 * stream-copy kernel whose rate is the measured bandwidth ceiling SURVEY.md
 * §8(d) asks the bench to report beside the 8 TB/s spec (float4 loads and
 * stores, several in flight per lane; bytes a multiple of 16, 16-byte aligned
 * device pointers), asynchronous on `stream` (a hipStream_t, NULL = default). */
RFA_API int rfa_stream_copy(void *dst, const void *src, size_t bytes, void *stream);
RFA_API int rfa_set_profiling(rfa_handle *h, int enable);
RFA_API int rfa_get_kernel_time(rfa_handle *h, double *total_ms, int64_t *launches);
/* Host-only helper (no device work): the waterfall shift in bins applied by
 * rfa_set_tuning for a retune by frequency_diff = last_frequency - frequency,
 * ((lastF - f) * (N / sampleRate.toFloat())).toInt() in fp32 with Kotlin's
 * truncating, saturating Float.toInt() (FftProcessor.kt:143,173,199). */
RFA_API int64_t rfa_retune_offset(int64_t frequency_diff, int n, int64_t sample_rate);
/* Name of the HIP kernel rfa_process launches for this handle's configuration
 * ("fft_wide_kernel" or "fft_rows_kernel"), as rocprofv3 reports it. */
RFA_API const char *rfa_main_kernel_name(const rfa_handle *h);

/* ------------------------------------------------------------------------
 * Demod-branch front end: NCO down-mix of raw IQ
 * bytes + decimating low-pass FIR, one handle per demodulated channel.
 * Replaces (app paths as above):
 *   IQConverter.mixPacketIntoSamplePacket        rfa_ddc_set_frequencies() +
 *     source/Signed8BitIQConverter.java:53-131,    rfa_ddc_process()
 *     Unsigned8BitIQConverter.java:53-131,
 *     Signed16BitIQConverter.kt:59-181, IQConverter.java:64-76
 *   Decimator.downsampling / FirFilter.filter    rfa_ddc_process()
 *     analyzer/Decimator.java:175-191, dsp/FirFilter.kt:63-107
 *   FirFilter.createLowPassTaps                  rfa_lowpass_taps()  (host only)
 *     dsp/FirFilter.kt:134-195, dsp/WindowFunctions.kt:44-52
 * The filter state (delay line, decimation counter) and the mixer's cosine
 * index carry over between calls exactly as in the reference, so one call on
 * a long buffer equals the reference run packet by packet.
 * ------------------------------------------------------------------------ */
typedef struct rfa_ddc rfa_ddc;

/* input_format: RFA_IN_S8 / RFA_IN_U8 / RFA_IN_S16LE are mixed then filtered;
 * RFA_IN_F32_INTERLEAVED is taken as already-mixed samples and only filtered
 * (the Decimator on a float SamplePacket).  Decimation = sample_rate /
 * output_sample_rate; taps = createLowPassTaps(decimation, 1, sample_rate,
 * 0.75 * out, 0.25 * out, 60) (Decimator.java:177-181).  RFA_ERR_INVALID where
 * the reference's filter design returns null. */
RFA_API int rfa_ddc_create(int device, int input_format, int32_t sample_rate, int32_t output_sample_rate,
                           rfa_ddc **out);
/* The same front end with the resampler the live app uses instead of the
 * Decimator (analyzer/Resampler.kt:102-110, dsp/RationalResampler.kt): the
 * ratio out/in reduced by limitDenominator(out, in, 10000), polyphase bank
 * from designResamplerTaps (Kaiser beta 7, fractionalBw 0.4, 500 taps per phase
 * at most), outputs in the reference's phase order.  Downsampling only
 * (RFA_ERR_UNSUPPORTED otherwise, as the reference's TODO states).
 * rfa_ddc_get_taps returns the prototype padded to a multiple of the
 * interpolation; rfa_ddc_get_ratio the reduced interpolation/decimation. */
RFA_API int rfa_ddc_create_resampler(int device, int input_format, int32_t sample_rate, int32_t output_sample_rate,
                                     rfa_ddc **out);
/* A FirFilter with the caller's taps and decimation (dsp/FirFilter.kt:34-110,
 * e.g. FirFilter.createLowPass): delay line of num_taps zeros, decimationCounter
 * 1, outputs sum taps[k] * delay[newest - k] with the JVM's separately rounded
 * products and sums.  input_format as in rfa_ddc_create (RFA_IN_F32_INTERLEAVED:
 * samples taken as they are; raw formats are mixed first). */
RFA_API int rfa_ddc_create_fir(int device, int input_format, int32_t sample_rate, const float *taps, int32_t num_taps,
                               int32_t decimation, rfa_ddc **out);
/* Enqueue on exactly `stream` (a hipStream_t; NULL restores the handle's own
 * stream).  Pending work of the previous stream is drained first. */
RFA_API int rfa_ddc_set_stream(rfa_ddc *d, void *stream);
RFA_API int rfa_ddc_get_ratio(const rfa_ddc *d, int32_t *interpolation, int32_t *decimation, int32_t *taps_per_output);
RFA_API int rfa_ddc_get_format(const rfa_ddc *d, int32_t *input_format);  /* rfa_input_format of the handle */
RFA_API int rfa_ddc_destroy(rfa_ddc *d);
RFA_API const char *rfa_ddc_last_error(const rfa_ddc *d);
/* Like IQConverter.setSampleRate + the Decimator's rebuild check: the mixer
 * table is invalidated; the filter is rebuilt (fresh delay line) only when the
 * integer decimation changes (Decimator.java:177-178). */
RFA_API int rfa_ddc_set_sample_rate(rfa_ddc *d, int32_t sample_rate);
/* mixFrequency = (int)(frequency - channel_frequency), folded by +sample_rate
 * when 0 or when sample_rate / |mix| > 500; the table (and the cosine index)
 * is regenerated only when the folded frequency changes. */
RFA_API int rfa_ddc_set_frequencies(rfa_ddc *d, int64_t frequency, int64_t channel_frequency);
/* n_samples complex samples of raw input at device address `in` -> the
 * decimated outputs at device out_re/out_im (planar float).  *n_out is set on
 * return (computed on the host); RFA_ERR_SIZE if it would exceed out_capacity
 * (nothing is consumed then).  Asynchronous on the handle's stream. */
RFA_API int rfa_ddc_process(rfa_ddc *d, const void *in, size_t n_samples, float *out_re, float *out_im,
                            size_t out_capacity, size_t *n_out);
/* Same with host buffers; synchronous. */
RFA_API int rfa_ddc_process_host(rfa_ddc *d, const void *in, size_t n_samples, float *out_re, float *out_im,
                                 size_t out_capacity, size_t *n_out);
RFA_API int rfa_ddc_synchronize(rfa_ddc *d);
RFA_API int rfa_ddc_get_stream(const rfa_ddc *d, void **stream);
/* Current design: taps (capacity floats), mixer cos/sin per time step
 * (capacity floats each, may be NULL), counts and folded mix frequency. */
RFA_API int rfa_ddc_get_taps(const rfa_ddc *d, float *taps, size_t capacity, int32_t *num_taps, int32_t *decimation);
RFA_API int rfa_ddc_get_mixer(const rfa_ddc *d, float *cos_t, float *sin_t, size_t capacity, int32_t *length,
                              int32_t *mix_frequency, int32_t *cosine_index);
/* Host-only filter design, FirFilter.createLowPassTaps with a Blackman window
 * (no device work).  *num_taps is always set; taps written when it fits. */
/* Host-only RationalResampler design: limitDenominator + designResamplerTaps
 * (RationalResampler.kt:165-235); the prototype taps before the polyphase split. */
RFA_API int rfa_resampler_design(int32_t output_rate, int32_t input_rate, int32_t max_denominator, float fractional_bw,
                                 int32_t max_taps, int32_t *interpolation, int32_t *decimation, float *taps,
                                 size_t capacity, int32_t *num_taps);
RFA_API int rfa_lowpass_taps(float gain, float sample_rate, float cutoff, float transition, float attenuation,
                             int32_t max_taps, float *taps, size_t capacity, int32_t *num_taps);

/* ------------------------------------------------------------------------
 * Front-end channel bank: K channels out of one raw
 * IQ stream per call.  Replaces K rfa_ddc handles fed the same bytes, i.e. K
 * times (app paths as above)
 *   IQConverter.mixPacketIntoSamplePacket        rfa_ddc_bank_set_frequencies() +
 *     (one table and cosine index per slot)        rfa_ddc_bank_process()
 *   Decimator.downsampling / Resampler.resample  rfa_ddc_bank_process()
 *     (one filter design, one delay line per slot)
 * The slots share input format, rates and therefore the filter (taps, ratio,
 * decimation counter); each owns its mixer (folded frequency, table, cosine
 * index) and its delay line.  Slot k produces, bit for bit, what an rfa_ddc
 * handle created with the same arguments and given the same calls produces.
 * The one deliberate difference: a slot whose mixer table would be empty
 * (rfa_ddc_mix_info reports length 0) is rejected by
 * rfa_ddc_bank_set_frequencies with RFA_ERR_UNSUPPORTED, where the single
 * handle silently produces nothing and does not advance -- that slot would
 * fall out of step with the filter clock the bank shares.
 * ------------------------------------------------------------------------ */
typedef struct rfa_ddc_bank rfa_ddc_bank;

#define RFA_DDC_BANK_MAX_CHANNELS 1024      /* n_channels above this: RFA_ERR_INVALID */
#define RFA_DDC_BANK_LAUNCH_CHANNELS 256    /* channels one kernel launch covers */
#define RFA_DEMOD_BANK_MAX_CHANNELS 1024    /* rfa_demod_bank_create (below): n_channels above this is RFA_ERR_INVALID */

/* resampler 0: the Decimator of rfa_ddc_create; 1: the Resampler of
 * rfa_ddc_create_resampler.  1 <= n_channels <= RFA_DDC_BANK_MAX_CHANNELS, fixed
 * for the bank's life.  RFA_IN_F32_INTERLEAVED is RFA_ERR_UNSUPPORTED (float
 * input arrives mixed: every slot would be the same channel).  Arguments are
 * checked before the device is looked for. */
RFA_API int rfa_ddc_bank_create(int device, int input_format, int32_t sample_rate, int32_t output_sample_rate,
                                int resampler, int32_t n_channels, rfa_ddc_bank **out);
RFA_API int rfa_ddc_bank_destroy(rfa_ddc_bank *b);
RFA_API const char *rfa_ddc_bank_last_error(const rfa_ddc_bank *b);
RFA_API int rfa_ddc_bank_get_channels(const rfa_ddc_bank *b, int32_t *n_channels);
/* rfa_ddc_set_sample_rate for every slot: all mixers become invalid; the filter
 * is rebuilt (every delay line zeroed, counters reset) under the same
 * conditions; on failure the old rate and filter stay. */
RFA_API int rfa_ddc_bank_set_sample_rate(rfa_ddc_bank *b, int32_t sample_rate);
/* rfa_ddc_set_frequencies(frequency, channel_frequency[k]) on every slot k
 * (channel_frequency has n_channels entries): a slot whose folded mix frequency
 * is unchanged keeps its cosine index, a changed one gets a new table and index
 * 0; delay lines are not touched.  All or nothing: every slot's table is
 * designed and checked first, and if one is rejected (empty table, see above)
 * no slot changes. */
RFA_API int rfa_ddc_bank_set_frequencies(rfa_ddc_bank *b, int64_t frequency, const int64_t *channel_frequency);
/* Upper bound, per channel, of the outputs of one call of n_samples. */
RFA_API int rfa_ddc_bank_max_outputs(const rfa_ddc_bank *b, size_t n_samples, size_t *n);
/* rfa_ddc_process for every slot: out_re / out_im are [n_channels][channel_stride]
 * device floats, slot k's outputs at k * channel_stride; *n_out is the count per
 * channel (the same for all).  RFA_ERR_STATE until every slot has a valid mixer;
 * RFA_ERR_SIZE when channel_stride is smaller than the count (nothing is
 * enqueued or consumed then); input pointer rules as rfa_ddc_process.  A call
 * too short for an output still advances delay lines and cosine indices.
 * Asynchronous on the bank's stream; no copy, allocation or synchronisation.
 * Up to RFA_DDC_BANK_LAUNCH_CHANNELS channels the call is two kernel launches
 * (filter, delay lines); a larger bank takes two per group of that many. */
RFA_API int rfa_ddc_bank_process(rfa_ddc_bank *b, const void *in, size_t n_samples, float *out_re, float *out_im,
                                 size_t channel_stride, size_t *n_out);
/* Same with host buffers; copies and synchronises. */
RFA_API int rfa_ddc_bank_process_host(rfa_ddc_bank *b, const void *in, size_t n_samples, float *out_re,
                                      float *out_im, size_t channel_stride, size_t *n_out);
/* Slot k's mixer as rfa_ddc_get_mixer reports it; RFA_ERR_STATE while invalid. */
RFA_API int rfa_ddc_bank_get_channel(const rfa_ddc_bank *b, int32_t k, int32_t *mix_frequency, int32_t *table_length,
                                     int32_t *cosine_index);
/* As rfa_ddc_get_ratio / _get_taps / _set_stream / _get_stream / _synchronize. */
RFA_API int rfa_ddc_bank_get_ratio(const rfa_ddc_bank *b, int32_t *interpolation, int32_t *decimation,
                                   int32_t *taps_per_output);
RFA_API int rfa_ddc_bank_get_taps(const rfa_ddc_bank *b, float *taps, size_t capacity, int32_t *num_taps,
                                  int32_t *decimation);
RFA_API int rfa_ddc_bank_set_stream(rfa_ddc_bank *b, void *stream);
RFA_API int rfa_ddc_bank_get_stream(const rfa_ddc_bank *b, void **stream);
RFA_API int rfa_ddc_bank_synchronize(rfa_ddc_bank *b);
/* Host only, no device needed: the folded mix frequency and the table length
 * rfa_ddc_set_frequencies would build for one channel (generateMixerLookupTable's
 * fold, IQConverter.calcOptimalCosineLength, IQConverter.java:64-76).  Length 0
 * is the empty table.  RFA_ERR_UNSUPPORTED for RFA_IN_F32_INTERLEAVED. */
RFA_API int rfa_ddc_mix_info(int input_format, int32_t sample_rate, int64_t frequency, int64_t channel_frequency,
                             int32_t *mix_frequency, int32_t *table_length);
/* Host only, no handle and no device needed: the workgroup tile plan every
 * rfa_ddc_process / rfa_ddc_bank_process call of such a filter launches with
 * (the same planning code the launch runs).  taps_per_output, interpolation and
 * decimation as rfa_ddc_get_ratio reports them (decimator / explicit FIR:
 * interpolation 1); table_length as rfa_ddc_get_mixer / rfa_ddc_mix_info report
 * it (0 for RFA_IN_F32_INTERLEAVED; a bank plans with its longest table).
 * plan receives RFA_DDC_PLAN_FIELDS values, indexed by rfa_ddc_plan_field.
 * RFA_ERR_INVALID for a count below 1 (table_length below 0) or a null plan;
 * RFA_ERR_UNSUPPORTED for a table rfa_ddc_set_frequencies would reject. */
enum rfa_ddc_plan_field {
    RFA_DDC_PLAN_OUTPUTS = 0,     /* P: decimated outputs per workgroup */
    RFA_DDC_PLAN_THREADS = 1,     /* workgroup size: P rounded up to a multiple of 64 */
    RFA_DDC_PLAN_CHUNK_TAPS = 2,  /* KC: taps per LDS pass (== taps_per_output when one pass does) */
    RFA_DDC_PLAN_CHUNKS = 3,      /* passes: ceil(taps_per_output / KC) */
    RFA_DDC_PLAN_PAD = 4,         /* 1: rows of RFA_DDC_PLAN_ROW samples at an odd pitch; 0: linear */
    RFA_DDC_PLAN_ROW = 5,         /* LDS row length in samples: max(1, decimation / interpolation) */
    RFA_DDC_PLAN_LDS_BYTES = 6,   /* dynamic LDS of one workgroup */
    RFA_DDC_PLAN_FIELDS = 7
};
RFA_API int rfa_ddc_tile_plan(int32_t taps_per_output, int32_t interpolation, int32_t decimation,
                              int32_t table_length, int32_t *plan);

/* ------------------------------------------------------------------------
 * Polyphase channelizer: all n_channels = M channels of the
 * uniform raster k * Fs / M out of one raw IQ stream per call, for a cost that
 * does not grow with the channel count.  For channels on a raster it replaces
 * the front-end channel bank above; a tuning (rfa_pfb_set_tuning, below) moves a
 * slot up to half a spacing off its raster centre, so any frequency list runs here
 * too.  Only a bit-for-bit match with the app's own Resampler stays with the bank.
 * With x[j] the converted input (s8: b/128, u8: (b-127.4f)/128, s16: s/32768,
 * float I,Q as it is; j counts samples since creation or reset, x[j] = 0 for
 * j < 0), real prototype taps h[0..T-1] and integer decimation D, output n is
 * due once sample i_n = n * D + D - 1 has been consumed (FirFilter's counter)
 * and channel k is
 *   y_k[n] = sum_t h[t] * x[i_n - t] * exp(-j 2 pi k (i_n - t) / M)
 * -- an NCO at k * Fs / M with absolute phase, the FIR, decimation by D.  A
 * tone at +k * Fs / M lands in channel k with gain sum(h); channels k >= M/2
 * are the negative offsets (k - M) * Fs / M.  It is computed as a fold
 *   u_n[r] = sum of h[t] * x[i_n - t] over the t with (i_n - t) mod M == r
 * (t ascending from 0, product and sum rounded separately) and one forward
 * M-point DFT over r.  An output's bits do not depend on how the stream is cut
 * into calls, on the channel selection or on the raw pointer's offset.
 * ------------------------------------------------------------------------ */
typedef struct rfa_pfb rfa_pfb;

#define RFA_PFB_MIN_CHANNELS 8
#define RFA_PFB_MAX_CHANNELS 4096
#define RFA_PFB_MAX_PHASES   16            /* num_taps <= 16 * n_channels */

/* Host only, no device needed: 1 where n_channels = 2^a 3^b 5^c within
 * RFA_PFB_MIN_CHANNELS .. RFA_PFB_MAX_CHANNELS, else 0. */
RFA_API int rfa_pfb_supported(int32_t n_channels);
/* input_format RFA_IN_S8 / _U8 / _S16LE / _F32_INTERLEAVED; 1 <= decimation <=
 * n_channels; 1 <= num_taps <= RFA_PFB_MAX_PHASES * n_channels (any length, not
 * only multiples of n_channels).  Arguments are checked before the device is
 * looked for: RFA_ERR_INVALID first, then RFA_ERR_UNSUPPORTED for an n_channels
 * rfa_pfb_supported rejects, and RFA_ERR_NODEVICE only for a valid request;
 * *out is NULL on every failure.  All channels are selected at creation. */
RFA_API int rfa_pfb_create(int device, int input_format, int32_t n_channels, int32_t decimation, const float *taps,
                           int32_t num_taps, rfa_pfb **out);
RFA_API int rfa_pfb_destroy(rfa_pfb *p);
RFA_API const char *rfa_pfb_last_error(const rfa_pfb *p);
/* The DFT's radices in stage order (each 2, 3, 4 or 5; their product is
 * n_channels): *count of them, copied where radices is given (RFA_ERR_SIZE when
 * cap is smaller).  Any output pointer may be NULL. */
RFA_API int rfa_pfb_get_plan(const rfa_pfb *p, int32_t *n_channels, int32_t *decimation, int32_t *num_taps,
                             int32_t *radices, int32_t cap, int32_t *count);
RFA_API int rfa_pfb_get_taps(const rfa_pfb *p, float *taps, size_t capacity, int32_t *num_taps);
/* Output slot j is channel channels[j]: entries in 0 .. n_channels - 1 in any
 * order, repeats allowed, 1 <= count <= n_channels; count 0 or a NULL list
 * selects all channels in natural order.  Uploaded between calls (drains the
 * stream).  An invalid list is RFA_ERR_INVALID and leaves the selection as it
 * was.  The selection changes which rows are written, never their values.
 * A successful call also removes any tuning (rfa_pfb_set_tuning): the slots it
 * creates are untuned. */
RFA_API int rfa_pfb_set_channels(rfa_pfb *p, const int32_t *channels, int32_t count);
RFA_API int rfa_pfb_get_channels(const rfa_pfb *p, int32_t *channels, size_t capacity, int32_t *count);
/* The exact output count per channel of the next call of n_samples:
 * floor((c + n_samples) / D) - floor(c / D) with c samples consumed so far. */
RFA_API int rfa_pfb_max_outputs(const rfa_pfb *p, size_t n_samples, size_t *n);
/* out_re / out_im are [selected][channel_stride] device floats, slot j's outputs
 * at j * channel_stride, time contiguous: the layout rfa_demod_bank_process
 * reads.  Only the selected rows' first *n_out floats are written.
 * RFA_ERR_SIZE when channel_stride is smaller than the count (nothing is
 * enqueued or consumed then).  A call too short for an output still advances
 * the history and the sample count; n_samples 0 is a no-op.  in may sit at any
 * sample boundary.  Asynchronous on the handle's stream: two kernel launches
 * (fold + DFT, history) whatever the channel count; no copy, allocation or
 * synchronisation. */
RFA_API int rfa_pfb_process(rfa_pfb *p, const void *in, size_t n_samples, float *out_re, float *out_im,
                            size_t channel_stride, size_t *n_out);
/* Same with host buffers; copies and synchronises. */
RFA_API int rfa_pfb_process_host(rfa_pfb *p, const void *in, size_t n_samples, float *out_re, float *out_im,
                                 size_t channel_stride, size_t *n_out);
/* History zeroed, sample count 0: the next call starts a new stream. */
RFA_API int rfa_pfb_reset(rfa_pfb *p);
/* As rfa_ddc_set_stream / _get_stream / _synchronize. */
RFA_API int rfa_pfb_set_stream(rfa_pfb *p, void *stream);
RFA_API int rfa_pfb_get_stream(const rfa_pfb *p, void **stream);
RFA_API int rfa_pfb_synchronize(rfa_pfb *p);

/* Rational-rate channelizer: the same M raster channels at
 * L / D times the input rate, 1 <= L <= D <= L * M, gcd(L, D) = 1, so a raster
 * runs at any source rate (RationalResampler's freedom, dsp/RationalResampler.kt).
 * x[j] as above; g[0..T-1] are the real prototype taps at rate L * Fs, g[s] = 0
 * for s >= T, Tp = ceil(T / L) taps per output.  Output n has phase
 * p_n = (n * D) mod L and newest sample m_n = floor(n * D / L), both from 64-bit
 * integers, and channel k is
 *   y_k[n] = sum_{t=0..Tp-1} g[p_n + t * L] * x[m_n - t] * exp(-j 2 pi k (m_n - t) / M)
 * computed as the fold
 *   u_n[r] = sum of g[p_n + t * L] * x[m_n - t] over the t with (m_n - t) mod M == r
 * (t ascending from 0, product and sum rounded separately) and the same forward
 * M-point DFT over r.  The NCO's phase is the integer input sample index, so
 * nothing drifts.  Output n is due once sample m_n has been consumed: after c
 * samples in total ceil(c * L / D) outputs have been produced (0 for c = 0), so
 * a call that takes the count from c0 to c1 yields ceil(c1 L / D) - ceil(c0 L / D)
 * per channel -- RationalResampler.resample's counter (ctr starts at 0,
 * RationalResampler.kt:101-150); channel 0 is that class's output on the unmixed
 * stream.  The bit-exactness rules of rfa_pfb_process hold unchanged; the window
 * of an output is always the Tp samples m_n - Tp + 1 .. m_n (a padding tap
 * multiplies its sample like any other, so a NaN there reaches the output).
 * L = 1 is allowed and keeps this convention, m_n = n * D: output 0 is due with
 * the first sample.  That is NOT rfa_pfb_create's i_n = n * D + D - 1; a handle
 * of rfa_pfb_create(.., D, ..) and one of rfa_pfb_create_rational(.., 1, D, ..)
 * sample the same filter D - 1 input samples apart. */
#define RFA_PFB_MAX_INTERPOLATION 64       /* every app rate to 48 / 96 / 384 kHz needs at most 48 / 125 */

/* As rfa_pfb_create with 1 <= interpolation <= RFA_PFB_MAX_INTERPOLATION,
 * interpolation <= decimation <= interpolation * n_channels, gcd 1, and
 * 1 <= num_taps <= RFA_PFB_MAX_PHASES * n_channels * interpolation.  Errors in
 * the same order: RFA_ERR_INVALID (gcd != 1 and interpolation > decimation
 * included), then RFA_ERR_UNSUPPORTED, then RFA_ERR_NODEVICE; *out is NULL on
 * every failure.  The handle is an rfa_pfb: every entry above works on it;
 * rfa_pfb_get_plan reports decimation D and num_taps T (the prototype's length),
 * rfa_pfb_get_taps the prototype, rfa_pfb_max_outputs / rfa_pfb_process the
 * count rule above, and the history holds Tp - 1 samples. */
RFA_API int rfa_pfb_create_rational(int device, int input_format, int32_t n_channels, int32_t interpolation,
                                    int32_t decimation, const float *taps, int32_t num_taps, rfa_pfb **out);
/* (L, D, Tp); on a handle of rfa_pfb_create (1, D, T).  Any pointer may be NULL. */
RFA_API int rfa_pfb_get_ratio(const rfa_pfb *p, int32_t *interpolation, int32_t *decimation,
                              int32_t *taps_per_output);
/* Host only, no handle and no device needed: the count rule, *n = ceil((consumed
 * + n_samples) L / D) - ceil(consumed L / D).  RFA_ERR_INVALID for a ratio
 * rfa_pfb_create_rational rejects on its own (L < 1, L > RFA_PFB_MAX_INTERPOLATION,
 * L > D, gcd != 1), a null n, or consumed + n_samples >= 2^53. */
RFA_API int rfa_pfb_rational_outputs(int32_t interpolation, int32_t decimation, uint64_t consumed, size_t n_samples,
                                     size_t *n);
/* Host only, no handle and no device needed: the workgroup tile plan every
 * rfa_pfb_process call of such a handle launches with (the same planning code
 * the launch runs).  interpolation 0 asks for the handle of rfa_pfb_create,
 * interpolation >= 1 for that of rfa_pfb_create_rational (1 included);
 * num_taps is the prototype's length T.  plan receives RFA_PFB_PLAN_FIELDS
 * values, indexed by rfa_pfb_plan_field.  RFA_ERR_INVALID for a null plan, a
 * negative interpolation and whatever the matching create entry refuses as
 * invalid, then RFA_ERR_UNSUPPORTED for an n_channels rfa_pfb_supported
 * rejects; nothing is written on an error. */
enum rfa_pfb_plan_field {
    RFA_PFB_PLAN_TIMES = 0,         /* NT: output times per workgroup, a power of two */
    RFA_PFB_PLAN_PITCH = 1,         /* Mp: LDS row pitch in points, n_channels | 1 */
    RFA_PFB_PLAN_RUN = 2,           /* samples a full workgroup depends on */
    RFA_PFB_PLAN_STAGED_RUN = 3,    /* 1: the run is staged in LDS; 0: the fold reads history and raw buffer */
    RFA_PFB_PLAN_STAGED_TAPS = 4,   /* rfa_pfb_create: 1 where the taps are staged (with the run), else 0;
                                       rational: the number of tap rows staged behind the run, 0 for none */
    RFA_PFB_PLAN_ROWS_BY_TIME = 5,  /* rational: 1 where the staged tap rows are indexed by output time
                                       (interpolation > NT), 0 where by phase or where none is staged */
    RFA_PFB_PLAN_STAGE_POINTS = 6,  /* 8-byte points of LDS in front of the DFT rows: staged run + taps */
    RFA_PFB_PLAN_LDS_BYTES = 7,     /* dynamic LDS of one workgroup as launched */
    RFA_PFB_PLAN_STAGES = 8,        /* DFT stages */
    RFA_PFB_PLAN_RADIX0 = 9,        /* their radices in stage order, RFA_PFB_PLAN_MAX_STAGES slots, 0 past the last */
    RFA_PFB_PLAN_FIELDS = 21
};
#define RFA_PFB_PLAN_MAX_STAGES 12
RFA_API int rfa_pfb_tile_plan(int32_t n_channels, int32_t interpolation, int32_t decimation, int32_t num_taps,
                              int32_t *plan);

/* Fine tuning: receivers at any frequency, not only on the
 * raster.  A handle of either create entry may carry a tuning: a denominator Q
 * and one integer step m_j per output slot j (a slot is an entry of the selection
 * set by rfa_pfb_set_channels).  With y_k[n] the output defined above and n the
 * absolute output index since creation or rfa_pfb_reset (a 64-bit count), slot j
 * writes
 *   i      = (n * m_j) mod Q                 mathematical mod, 0 <= i < Q, exact in integers
 *   (c, s) = W[i]                            W[i] = (float cos(2 pi i / Q), float sin(2 pi i / Q))
 *   z_re   = y_re * c + y_im * s             fp32, both products and the sum rounded separately
 *   z_im   = y_im * c - y_re * s
 * that is z = y * exp(-j 2 pi m_j n / Q): a signal m_j * Fout / Q Hz above the
 * raster centre of channels[j] lands at DC (Fout: the output rate).  The output
 * rate is several times the raster spacing, so a prototype with a pass band of
 * half a spacing plus the channel's width lets any frequency through its nearest
 * raster channel, and the demodulator's own filter selects the channel.
 * A slot with m_j == 0 is written untouched, with no multiply: NaN, inf and every
 * bit of it are those of an untuned handle.  The phase is a function of n alone:
 * it does not depend on how the stream is cut into calls and there is no per-slot
 * state, so nothing drifts; rfa_pfb_reset restarts n at 0 and keeps the tuning.
 * W is built once on the host in double, the angle first reduced by symmetry to
 * the first octant, each value rounded to float once: W[0] = (1, 0) exactly and,
 * where 4 divides Q, W[Q/4] = (0, 1), W[Q/2] = (-1, 0), W[3Q/4] = (0, -1) exactly.
 * One table of Q entries (8 Q bytes) is shared by all slots and uploaded with the
 * tuning. */
#define RFA_PFB_TUNE_MAX_STEPS (1 << 20)   /* Q at most: 1 Hz steps at up to 1.048 MHz output rate */

/* 1 <= q <= RFA_PFB_TUNE_MAX_STEPS, count equal to the number of currently
 * selected slots, -q < steps[j] < q.  q == 0 or steps == NULL removes the tuning
 * (with q == 0 and steps given, count is still checked).  An invalid request is
 * RFA_ERR_INVALID and leaves the previous tuning as it was.  Uploaded between
 * calls (drains the stream; may allocate) and in force from the next output.  A
 * call of rfa_pfb_process on a tuned handle is still two launches -- the rotation
 * is part of the store of the fold + DFT kernel -- and allocates nothing; a
 * handle without a tuning launches the kernels it launched before this entry
 * existed.  rfa_pfb_set_channels removes the tuning. */
RFA_API int rfa_pfb_set_tuning(rfa_pfb *p, int32_t q, const int32_t *steps, int32_t count);
/* The denominator and the steps as given; *q = 0 and *count = 0 when there is no
 * tuning.  RFA_ERR_SIZE where steps is given and capacity is smaller than the
 * count.  Any output pointer may be NULL. */
RFA_API int rfa_pfb_get_tuning(const rfa_pfb *p, int32_t *q, int32_t *steps, size_t capacity, int32_t *count);
/* Host only, no handle and no device needed: *i = (n * step) mod q for n < 2^53,
 * by the very function the kernel calls (a multiply-high reduction, no division).
 * RFA_ERR_INVALID for q outside 1 .. RFA_PFB_TUNE_MAX_STEPS, |step| >= q,
 * n >= 2^53 or a null i. */
RFA_API int rfa_pfb_tuning_index(int32_t q, int32_t step, uint64_t n, int32_t *i);
/* Host only: the table W a handle uploads for q, cos_t[i] and sin_t[i] for
 * 0 <= i < q.  RFA_ERR_INVALID for q out of range or a null array, RFA_ERR_SIZE
 * for capacity < q. */
RFA_API int rfa_pfb_tuning_table(int32_t q, float *cos_t, float *sin_t, size_t capacity);

/* ------------------------------------------------------------------------
 * Demodulator: quadrature-rate IQ (what rfa_ddc_process writes, planar float
 * on the device) -> 48 kHz float audio.  One handle is one Demodulator with
 * its AudioSink.  Replaces (app paths as above):
 *   Demodulator.run's per-packet chain           rfa_demod_process()
 *     analyzer/Demodulator.kt:151-187
 *   applyUserFilter / FirFilter.filter           rfa_demod_process()
 *     analyzer/Demodulator.kt:215-240, dsp/FirFilter.kt:63-107
 *   demodulateFM / AM / SSB / CW                 rfa_demod_process()
 *     analyzer/Demodulator.kt:251-403
 *   ComplexFirFilter.filter                      rfa_demod_process()
 *     dsp/ComplexFirFilter.java:123-170
 *   ComplexFirFilter.createBandPass              rfa_bandpass_taps()  (host only)
 *     dsp/ComplexFirFilter.java:186-278
 *   AudioSink's filters and applyAudioFilter     rfa_demod_process()
 *     analyzer/AudioSink.java:94-97,215-237, dsp/FirFilter.kt:121-163
 *   DemodulationMode's rates and widths          rfa_demod_mode_info() (host only)
 *     analyzer/Demodulator.kt:52-61
 * A call carries n_samples split into packets of packet_samples (the last one
 * may be short; 0 = one packet; n_samples 0 = one empty packet) and equals the
 * reference run packet by packet: AM's mean and the AGC are per-packet
 * quantities.  The filters' delay lines and counters, carryOverSamples and
 * lastMax carry over between packets, calls and mode changes as there.
 * AM, LSB, USB and CW audio is bit-exact against the restated chain; FM differs
 * only where the device's double atan2 rounds differently from the host's.
 * ------------------------------------------------------------------------ */
typedef struct rfa_demod rfa_demod;
enum rfa_demod_mode { RFA_DEMOD_OFF, RFA_DEMOD_AM, RFA_DEMOD_NFM, RFA_DEMOD_WFM, RFA_DEMOD_LSB, RFA_DEMOD_USB,
                      RFA_DEMOD_CW };
enum rfa_demod_taps { RFA_DEMOD_TAPS_USER, RFA_DEMOD_TAPS_BANDPASS, RFA_DEMOD_TAPS_AUDIO1, RFA_DEMOD_TAPS_AUDIO2 };

/* Host only: quadrature rate and channel width limits of a mode (any pointer may be NULL). */
RFA_API int rfa_demod_mode_info(int mode, int32_t *quadrature_rate, int32_t *min_width, int32_t *max_width,
                                int32_t *default_width);
/* Host only: ComplexFirFilter.createBandPass's taps with its float/double
 * promotions.  RFA_ERR_INVALID where it returns null; *num_taps is always set,
 * re/im (either may be NULL) written when capacity suffices. */
RFA_API int rfa_bandpass_taps(float gain, float fs, float lo, float hi, float transition, float attenuation,
                              float *re, float *im, size_t capacity, int32_t *num_taps);
/* A Demodulator with demodulationMode = mode (channel width = the mode's
 * default, volume 1) and a fresh AudioSink.  RFA_ERR_NODEVICE without a GPU. */
RFA_API int rfa_demod_create(int device, int mode, rfa_demod **out);
RFA_API int rfa_demod_destroy(rfa_demod *d);
RFA_API const char *rfa_demod_last_error(const rfa_demod *d);
/* demodulationMode's setter (Demodulator.kt:96-100): width := the mode's
 * default; every filter, AGC and carry-over state is kept. */
RFA_API int rfa_demod_set_mode(rfa_demod *d, int mode);
RFA_API int rfa_demod_get_mode(const rfa_demod *d, int32_t *mode);
/* channelWidth's setter: coerced into the mode's [min, max] (Demodulator.kt:75).
 * The user filter is rebuilt by the next packet when its cut-off differs (:217). */
RFA_API int rfa_demod_set_channel_width(rfa_demod *d, int32_t w);
RFA_API int rfa_demod_get_channel_width(const rfa_demod *d, int32_t *w);
RFA_API int rfa_demod_set_volume(rfa_demod *d, float v);      /* audioVolumeLevel */
/* enable 0: the output is the Demodulator's audioBuffer after the volume, at
 * the packet rate, and the AudioSink's filters see nothing. */
RFA_API int rfa_demod_set_audio_sink(rfa_demod *d, int enable);
/* Device pointers, asynchronous on the handle's stream.  *n_audio is computed on
 * the host; RFA_ERR_SIZE if it exceeds capacity (nothing is consumed then).
 * RFA_DEMOD_OFF: no output and no state change. */
RFA_API int rfa_demod_process(rfa_demod *d, const float *re, const float *im, size_t n_samples,
                              size_t packet_samples, float *audio, size_t capacity, size_t *n_audio);
/* Same with host buffers; synchronous. */
RFA_API int rfa_demod_process_host(rfa_demod *d, const float *re, const float *im, size_t n_samples,
                                   size_t packet_samples, float *audio, size_t capacity, size_t *n_audio);
/* Exactly what the next rfa_demod_process of n_samples would write. */
RFA_API int rfa_demod_max_outputs(const rfa_demod *d, size_t n_samples, size_t *n);
/* which: rfa_demod_taps.  The user and band-pass filters exist once a packet
 * built them (0 taps before); im is zero for the real filters. */
RFA_API int rfa_demod_get_taps(const rfa_demod *d, int which, float *re, float *im, size_t capacity,
                               int32_t *num_taps, int32_t *decimation);
/* lastMax and carryOverSamplesRe/Im; drains the stream. */
RFA_API int rfa_demod_get_state(rfa_demod *d, float *last_max, float *carry_re, float *carry_im);
/* The signal path of a freshly created Demodulator + AudioSink: no user or
 * band-pass filter, zero carry-over and lastMax, empty audio delay lines.
 * Mode, width, volume and the audio-sink switch stay. */
RFA_API int rfa_demod_reset(rfa_demod *d);
/* As rfa_ddc_set_stream / _get_stream / _synchronize. */
RFA_API int rfa_demod_set_stream(rfa_demod *d, void *stream);
RFA_API int rfa_demod_get_stream(const rfa_demod *d, void **stream);
RFA_API int rfa_demod_synchronize(rfa_demod *d);

/* ------------------------------------------------------------------------
 * Demodulator bank: n_channels Demodulators (each with its AudioSink) in one
 * handle, on one stream and with one set of launches per call -- four kernels
 * and one copy of the slots' launch records, whatever n_channels.  Slot k
 * computes, bit for bit, what an rfa_demod handle computes when it is given the
 * same settings and the same calls; the per-slot entries have the single
 * handle's semantics (a mode change keeps every state, the width is coerced
 * into the mode's limits, a reset touches that slot alone).  Modes of different
 * quadrature rates may share a bank: it sees samples, not rates.  A slot index
 * outside 0 .. n_channels-1 is RFA_ERR_INVALID.
 * ------------------------------------------------------------------------ */
typedef struct rfa_demod_bank rfa_demod_bank;

/* modes[n_channels]: rfa_demod_mode of every slot; 1 <= n_channels <=
 * RFA_DEMOD_BANK_MAX_CHANNELS.  Arguments are checked before the device is
 * looked for: RFA_ERR_INVALID comes first, RFA_ERR_NODEVICE (with *out NULL)
 * only for a valid request. */
RFA_API int rfa_demod_bank_create(int device, const int32_t *modes, int32_t n_channels, rfa_demod_bank **out);
RFA_API int rfa_demod_bank_destroy(rfa_demod_bank *b);
RFA_API const char *rfa_demod_bank_last_error(const rfa_demod_bank *b);
RFA_API int rfa_demod_bank_get_channels(const rfa_demod_bank *b, int32_t *n_channels);
/* As rfa_demod_set_mode ... rfa_demod_reset, on slot k. */
RFA_API int rfa_demod_bank_set_mode(rfa_demod_bank *b, int32_t k, int mode);
RFA_API int rfa_demod_bank_get_mode(const rfa_demod_bank *b, int32_t k, int32_t *mode);
RFA_API int rfa_demod_bank_set_channel_width(rfa_demod_bank *b, int32_t k, int32_t w);
RFA_API int rfa_demod_bank_get_channel_width(const rfa_demod_bank *b, int32_t k, int32_t *w);
RFA_API int rfa_demod_bank_set_volume(rfa_demod_bank *b, int32_t k, float v);
RFA_API int rfa_demod_bank_set_audio_sink(rfa_demod_bank *b, int32_t k, int enable);
RFA_API int rfa_demod_bank_get_taps(const rfa_demod_bank *b, int32_t k, int which, float *re, float *im,
                                    size_t capacity, int32_t *num_taps, int32_t *decimation);
RFA_API int rfa_demod_bank_get_state(rfa_demod_bank *b, int32_t k, float *last_max, float *carry_re,
                                     float *carry_im);
RFA_API int rfa_demod_bank_reset(rfa_demod_bank *b, int32_t k);
/* n[n_channels]: exactly what the next rfa_demod_bank_process of n_samples would write per slot. */
RFA_API int rfa_demod_bank_max_outputs(const rfa_demod_bank *b, size_t n_samples, size_t *n);
/* Device pointers, asynchronous on the bank's stream.  Slot k reads n_samples
 * floats at re + k*channel_stride and im + k*channel_stride and writes
 * n_audio[k] floats at audio + k*audio_stride; the strides are in floats and
 * audio_stride is every slot's capacity; channel_stride below n_samples (rows
 * that overlap) is RFA_ERR_INVALID where n_channels > 1.  If any slot would write more, the call
 * returns RFA_ERR_SIZE and consumes nothing in any slot.  A slot in
 * RFA_DEMOD_OFF writes nothing, reports 0 and keeps its state.  Stale user and
 * band-pass filters of all slots are designed first (a rejected design fails the
 * call with no slot changed) and uploaded behind one synchronisation; a call
 * that rebuilds nothing and grows no scratch neither allocates nor waits for the
 * device, except for the copy of an earlier call's records where more than 8
 * calls are queued. */
RFA_API int rfa_demod_bank_process(rfa_demod_bank *b, const float *re, const float *im, size_t channel_stride,
                                   size_t n_samples, size_t packet_samples, float *audio, size_t audio_stride,
                                   size_t *n_audio /* [n_channels] */);
/* Same with host buffers; synchronous. */
RFA_API int rfa_demod_bank_process_host(rfa_demod_bank *b, const float *re, const float *im, size_t channel_stride,
                                        size_t n_samples, size_t packet_samples, float *audio, size_t audio_stride,
                                        size_t *n_audio /* [n_channels] */);
/* As rfa_ddc_set_stream / _get_stream / _synchronize. */
RFA_API int rfa_demod_bank_set_stream(rfa_demod_bank *b, void *stream);
RFA_API int rfa_demod_bank_get_stream(const rfa_demod_bank *b, void **stream);
RFA_API int rfa_demod_bank_synchronize(rfa_demod_bank *b);

/* ------------------------------------------------------------------------
 * Squelch bank: a level meter on the quadrature rows of n_channels slots and
 * the reference's squelch rule per slot (analyzer/Scheduler.kt:52,161-165,237;
 * database/AppStateRepository.kt:318-324).
 *
 * Level.  A call gives slot k the n samples (re[i], im[i]) of its row:
 *     term[i] = re[i]*re[i] + im[i]*im[i]     fp32, products and sum rounded separately
 *     s_k     = sum of term[i], i < n         accumulated in double on the device
 *     level_k = (float)(5 * log10(s_k / n))   in double on the host
 * the reference's magnitude-dB: a tone of amplitude A reads 10*log10(A).  s_k = 0
 * gives -inf, a NaN sample NaN (never satisfied), +inf satisfies; n = 0 keeps the
 * slot's previous level, RFA_SQUELCH_INITIAL_LEVEL at first.  Which samples a
 * lane and a tile sum, and the order of every addition, depend on i and n alone
 * -- not on the row's address, channel_stride or n_channels -- and there are no
 * atomics: s_k is bit-identical run to run and for any pointer offset.
 *
 * Rule, per slot, once per call (n = 0 included):
 *     satisfied = !enabled || level > threshold
 *     if (satisfied) counter = 0; else if (counter < debounce) counter++;
 *     open = satisfied || counter < debounce
 * A slot is created disabled (always open) with counter 0.
 *
 * Acting on a closed gate.  The demodulator bank passes over a slot in
 * RFA_DEMOD_OFF: nothing written, a count of 0, every state and filter counter
 * kept, no filter designed.  To withhold a call from slot k, note its mode and
 * width, switch it to RFA_DEMOD_OFF, and on release set the mode and then the
 * width again (a mode change keeps every state but sets the mode's default
 * width; a filter is stale by mode and width alone).  The slot then equals an
 * rfa_demod handle that was given only the calls made while it was on.
 * ------------------------------------------------------------------------ */
typedef struct rfa_squelch rfa_squelch;

#define RFA_SQUELCH_MAX_CHANNELS 1024          /* n_channels above this: RFA_ERR_INVALID */
#define RFA_SQUELCH_DEFAULT_DEBOUNCE 50        /* Scheduler.kt:52 */
#define RFA_SQUELCH_INITIAL_LEVEL (-999.0f)    /* the reference's initial averageSignalStrength */
#define RFA_SQUELCH_ONE_LAUNCH_MAX 16384       /* n_samples up to this: one launch; above: partials + fold */
#define RFA_SQUELCH_TILE 16384                 /* samples of one partials workgroup */

/* Host only, no device.  The level of a sum over n samples (`previous` for n = 0) and one
 * step of the rule (returns open; *counter is updated; a negative debounce counts as 0). */
RFA_API float rfa_squelch_level(double sum, size_t n, float previous);
RFA_API int rfa_squelch_step(int satisfied, int32_t debounce, int32_t *counter);

/* 1 <= n_channels <= RFA_SQUELCH_MAX_CHANNELS; arguments are checked before the
 * device is looked for (as rfa_demod_bank_create). */
RFA_API int rfa_squelch_create(int device, int32_t n_channels, rfa_squelch **out);
RFA_API int rfa_squelch_destroy(rfa_squelch *s);
RFA_API const char *rfa_squelch_last_error(const rfa_squelch *s);
RFA_API int rfa_squelch_get_channels(const rfa_squelch *s, int32_t *n_channels);
/* Slot k: enabled != 0 gates on level > threshold_db (a NaN threshold is RFA_ERR_INVALID). */
RFA_API int rfa_squelch_set(rfa_squelch *s, int32_t k, int enabled, float threshold_db);
RFA_API int rfa_squelch_get(const rfa_squelch *s, int32_t k, int32_t *enabled, float *threshold_db);
/* The handle's debounce, 0 allowed, negative RFA_ERR_INVALID; counters above a new, smaller
 * debounce are clipped to it. */
RFA_API int rfa_squelch_set_debounce(rfa_squelch *s, int32_t debounce);
RFA_API int rfa_squelch_get_debounce(const rfa_squelch *s, int32_t *debounce);
/* Counters to 0, levels to RFA_SQUELCH_INITIAL_LEVEL, sums to 0; the settings stay. */
RFA_API int rfa_squelch_reset(rfa_squelch *s);
/* Device pointers; planar rows channel_stride floats apart (the layout of
 * rfa_ddc_bank_process, rfa_pfb_process and rfa_demod_bank_process).  Enqueues the
 * level kernel(s) and one copy of the n_channels sums on the handle's stream, waits
 * for that copy alone (an event, not the stream), computes the levels, steps the rule
 * and fills level_db[n_channels] and open[n_channels] (host arrays, either may be NULL).
 * A steady-state call allocates nothing.  channel_stride below n_samples where
 * n_channels > 1, or a NULL row with n_samples > 0, is RFA_ERR_INVALID; on any error
 * counters and levels are unchanged. */
RFA_API int rfa_squelch_process(rfa_squelch *s, const float *re, const float *im, size_t channel_stride,
                                size_t n_samples, float *level_db, uint8_t *open);
/* Same with host rows. */
RFA_API int rfa_squelch_process_host(rfa_squelch *s, const float *re, const float *im, size_t channel_stride,
                                     size_t n_samples, float *level_db, uint8_t *open);
/* The last call's values, [n_channels] each; any pointer may be NULL. */
RFA_API int rfa_squelch_get_state(const rfa_squelch *s, double *sums, float *level_db, int32_t *counter,
                                  uint8_t *open);
/* As rfa_ddc_set_stream / _get_stream / _synchronize. */
RFA_API int rfa_squelch_set_stream(rfa_squelch *s, void *stream);
RFA_API int rfa_squelch_get_stream(const rfa_squelch *s, void **stream);
RFA_API int rfa_squelch_synchronize(rfa_squelch *s);

/* ------------------------------------------------------------------------
 * Frequency meter bank: where the signal of each of n_channels slots sits
 * relative to the slot's centre, from the quadrature rows the squelch bank
 * reads.  The reference tunes one channel by hand and has nothing like it.
 *
 * A call gives slot k the n samples x[i] = (re[i], im[i]) of its row and
 * produces the lag-1 autocorrelation
 *     R1 = sum of x[i] * conj(x[i-1])
 *     R1_re = sum (re[i]*re[i-1] + im[i]*im[i-1])
 *     R1_im = sum (im[i]*re[i-1] - re[i]*im[i-1])
 * as two doubles: every product is formed in double from the float inputs (and
 * is exact), a term is their sum rounded once, the terms are accumulated in
 * double.  x[-1] is the slot's last sample of the previous call, kept on the
 * device with a valid flag; without a valid one the term for i = 0 is left out.
 * The number of terms of the call -- n, or n - 1 without a predecessor, 0 for
 * n = 0 -- is reported per slot.  A carrier f Hz above the slot's centre gives
 * arg R1 = 2 pi f / rate (rfa_freq_error_hz), unambiguous for |f| < rate / 2.
 * A non-finite sample makes its slot's sums non-finite and touches no other slot.
 *
 * Which terms a lane and a tile sum, and the order of every addition, depend on
 * i and n alone -- not on the row's address, channel_stride or n_channels -- and
 * there are no atomics: a slot's sums are a function of its values, n and the
 * carried sample, bit for bit.  n up to RFA_FREQ_TILE is one launch, above that
 * a partials launch and a fold launch; n = 0 launches nothing, gives zero sums
 * and keeps the carry.
 * ------------------------------------------------------------------------ */
typedef struct rfa_freq rfa_freq;

#define RFA_FREQ_MAX_CHANNELS 1024             /* n_channels above this: RFA_ERR_INVALID */
#define RFA_FREQ_TILE 16384                    /* samples of one workgroup; n up to this: one launch */

/* Host only, no device: atan2(r1_im, r1_re) * rate / (2 pi).  0 for R1 = 0, NaN where a
 * sum is not finite. */
RFA_API double rfa_freq_error_hz(double r1_re, double r1_im, double rate);

/* 1 <= n_channels <= RFA_FREQ_MAX_CHANNELS; arguments are checked before the device is
 * looked for (as rfa_squelch_create).  No slot has a carry at first. */
RFA_API int rfa_freq_create(int device, int32_t n_channels, rfa_freq **out);
RFA_API int rfa_freq_destroy(rfa_freq *f);
RFA_API const char *rfa_freq_last_error(const rfa_freq *f);
RFA_API int rfa_freq_get_channels(const rfa_freq *f, int32_t *n_channels);
/* Drops slot k's carry (k = -1: every slot's): its next call starts without a predecessor.
 * For a slot whose phase is about to jump, such as one that was retuned.  A clear of the
 * flag enqueued on the handle's stream, no synchronisation. */
RFA_API int rfa_freq_break(rfa_freq *f, int32_t k);
/* Drops every carry and the last results (sums and terms read 0). */
RFA_API int rfa_freq_reset(rfa_freq *f);
/* Device pointers; planar rows channel_stride floats apart (the layout of
 * rfa_squelch_process).  Asynchronous: enqueues the launch(es), one copy of the
 * 2 * n_channels sums into pinned memory and an event on the handle's stream, and returns.
 * A steady-state call allocates nothing.  channel_stride below n_samples where
 * n_channels > 1, or a NULL row with n_samples > 0, is RFA_ERR_INVALID. */
RFA_API int rfa_freq_process(rfa_freq *f, const float *re, const float *im, size_t channel_stride,
                             size_t n_samples);
/* Waits for the last rfa_freq_process's event alone (not the stream) and hands out that call's
 * sums and term counts, [n_channels] each; any pointer may be NULL.  Without a call since
 * the last collect it waits for nothing and repeats the values. */
RFA_API int rfa_freq_collect(rfa_freq *f, double *r1_re, double *r1_im, int64_t *terms);
/* rfa_freq_process with host rows, then rfa_freq_collect: synchronous. */
RFA_API int rfa_freq_process_host(rfa_freq *f, const float *re, const float *im, size_t channel_stride,
                                  size_t n_samples, double *r1_re, double *r1_im, int64_t *terms);
/* As rfa_ddc_set_stream / _get_stream / _synchronize. */
RFA_API int rfa_freq_set_stream(rfa_freq *f, void *stream);
RFA_API int rfa_freq_get_stream(const rfa_freq *f, void **stream);
RFA_API int rfa_freq_synchronize(rfa_freq *f);

/* ---------------------------------------------------------------------------
 * Tone meter bank (extension): what a CTCSS tone squelch reads of every slot's audio
 *
 * The sub-audible tone under the voice (CTCSS, 67.0 ... 254.1 Hz, neighbours down to
 * 2.3 Hz apart) tells the users of a shared channel apart.  The device sums, per slot,
 * the audio row against up to three probe frequencies; the host turns the sums into a
 * quality (rfa_tone_quality) and decides (demod.ToneRule).  The reference has one
 * channel, squelched by hand, and nothing like this.
 *
 * Audio at sample_rate Hz (an integer, RFA_TONE_MIN_RATE ... RFA_TONE_MAX_RATE), M =
 * 10 * sample_rate.  A probe is a frequency in tenths of a hertz, int32 f10, 0 = unused,
 * else 1 <= f10 < 5 * sample_rate; slot k has three: probe 0 the wanted tone, 1 and 2
 * guards.  The phasor table W[p] = (cos, sin)(2 pi p / M), p = 0 ... M-1, is filled once
 * at creation in double by the host's libm (rfa_tone_phasor is the function that fills
 * it).  Every slot has a sample counter base_k, kept on the host modulo M, 0 at first;
 * sample i of a call meets, for probe j, W[p], p = (f10_j * (base_k + i)) mod M in 64-bit
 * integers, and the call advances base_k by the slot's n.  A row cut into calls anywhere
 * meets the phasors of the row given whole.
 *
 * Sums of slot k and one call of n_k samples a[i], RFA_TONE_SUMS doubles:
 *     [2j]   Sc_j = sum (double)a[i] * W[p_j(i)].cos      j = 0, 1, 2
 *     [2j+1] Ss_j = sum (double)a[i] * W[p_j(i)].sin
 *     [6]    P    = sum (double)a[i] * (double)a[i]       (every product exact)
 *     [7]    S1   = sum (double)a[i]
 * every product rounded once and not contracted with the addition; the two sums of an
 * unused probe read +0.0.  A non-finite sample makes its slot's sums non-finite and
 * touches no other slot.  The additions follow the summation plan of the other meters
 * (tiles of RFA_TONE_TILE) with the slot's own n_k: a slot's sums are a function of its
 * values, n_k, its probes and base_k alone, bit for bit.  Every n_k up to RFA_TONE_TILE
 * is one launch; otherwise a partials launch sized by the largest n_k and a fold launch.
 * A slot with n_k = 0 gets zero sums; a call whose counts are all 0 launches nothing.
 * ------------------------------------------------------------------------ */
typedef struct rfa_tone rfa_tone;

#define RFA_TONE_MAX_CHANNELS 1024             /* n_channels above this: RFA_ERR_INVALID */
#define RFA_TONE_MIN_RATE 8000
#define RFA_TONE_MAX_RATE 384000
#define RFA_TONE_PROBES 3
#define RFA_TONE_SUMS 8                        /* doubles per slot and call */
#define RFA_TONE_TILE 16384                    /* samples of one workgroup; every n_k up to this: one launch */

/* Host only, no device: W[p] of the table for sample_rate, cos(2 pi p / M) and sin of the same
 * angle, the angle formed in double as ((2 pi) * p) / M.  RFA_ERR_INVALID for a rate outside
 * the range, p outside 0 ... M-1 or a NULL pointer. */
RFA_API int rfa_tone_phasor(int32_t sample_rate, int64_t p, double *c, double *s);
/* Host only: 2 * (sc^2 + ss^2) / (n * p - s1^2), the share of the row's AC power that is
 * coherent at the probe (1 for a pure tone at the probe over whole periods).  0 where the
 * denominator is <= 0, NaN where sc, ss, p or s1 is not finite. */
RFA_API double rfa_tone_quality(double sc, double ss, double p, double s1, int64_t n);

/* 1 <= n_channels <= RFA_TONE_MAX_CHANNELS and a rate in range; arguments are checked before
 * the device is looked for.  No slot has a probe at first. */
RFA_API int rfa_tone_create(int device, int32_t n_channels, int32_t sample_rate, rfa_tone **out);
RFA_API int rfa_tone_destroy(rfa_tone *t);
RFA_API const char *rfa_tone_last_error(const rfa_tone *t);
RFA_API int rfa_tone_get_channels(const rfa_tone *t, int32_t *n_channels, int32_t *sample_rate);
/* Slot k's probes, f10[RFA_TONE_PROBES], from the next call on; the sample counter stays. */
RFA_API int rfa_tone_set_probes(rfa_tone *t, int32_t k, const int32_t *f10);
RFA_API int rfa_tone_get_probes(const rfa_tone *t, int32_t k, int32_t *f10);
/* Slot k's sample counter (k = -1: every slot's) back to 0.  Host only. */
RFA_API int rfa_tone_break(rfa_tone *t, int32_t k);
/* Every counter to 0 and the last results to 0; the probes stay. */
RFA_API int rfa_tone_reset(rfa_tone *t);
/* Device rows audio_stride floats apart, host counts n_audio[n_channels] (what
 * rfa_demod_bank_process returns).  Asynchronous: the call's records (counts, counters,
 * probes) go through a ring of pinned entries guarded by events, then the launch(es), one
 * copy of the RFA_TONE_SUMS * n_channels sums into pinned memory and an event, all on the
 * handle's stream.  A steady-state call allocates nothing and waits for nothing.  A count
 * above audio_stride where n_channels > 1, or a NULL row or count array with any count
 * > 0, is RFA_ERR_INVALID; nothing is consumed on an error. */
RFA_API int rfa_tone_process(rfa_tone *t, const float *audio, size_t audio_stride, const size_t *n_audio);
/* Waits for the last rfa_tone_process's event alone and hands out that call's sums,
 * [RFA_TONE_SUMS][n_channels], and counts, [n_channels]; either may be NULL.  Without a
 * call since the last collect it waits for nothing and repeats the values. */
RFA_API int rfa_tone_collect(rfa_tone *t, double *sums, int64_t *n);
/* rfa_tone_process with host rows, then rfa_tone_collect: synchronous. */
RFA_API int rfa_tone_process_host(rfa_tone *t, const float *audio, size_t audio_stride, const size_t *n_audio,
                                  double *sums, int64_t *n);
/* As rfa_ddc_set_stream / _get_stream / _synchronize. */
RFA_API int rfa_tone_set_stream(rfa_tone *t, void *stream);
RFA_API int rfa_tone_get_stream(const rfa_tone *t, void **stream);
RFA_API int rfa_tone_synchronize(rfa_tone *t);

/* ---------------------------------------------------------------------------
 * Code meter bank (extension): what a DCS code squelch reads of every slot's audio
 *
 * DCS (digital-coded squelch, CDCSS) is a 23-bit word sent continuously under the voice
 * at 134.4 bit/s = 672/5 Hz, NRZ, bit 0 first: bits 0 ... 8 the 9-bit code (three octal
 * digits), bits 9 ... 11 = 0, 0, 1, bits 12 ... 22 the parity of the systematic Golay
 * (23,12) code with generator 0xC75 (rfa_code_word).  The device sums, per slot, the
 * quantised audio over sub-cells, RFA_CODE_SUBCELLS to the bit; the host carries an
 * incomplete last sub-cell to the next call (rfa_code_merge) and correlates cells with
 * the wanted word (demod.CodeRule).  The reference has nothing like this.
 *
 * Audio at sample_rate Hz (an integer, RFA_CODE_MIN_RATE ... RFA_CODE_MAX_RATE).  Every
 * slot has a sample counter g, 0 at first and after rfa_code_break, limited to
 * g <= 2^48 (672 * RFA_CODE_SUBCELLS * g stays below 2^61; a call that would pass the
 * limit is RFA_ERR_INVALID).  Sample g belongs to sub-cell
 *     s(g) = floor(672 * RFA_CODE_SUBCELLS * g / (5 * sample_rate))    in 64-bit integers
 * and contributes
 *     q(a) = llrint((double)a * 2^24)                                  ties to even
 * or 0 where a is not finite or |a| >= 2^15; such a sample is counted in the slot's bad
 * count of the call instead.  A call with counter g0 and n_k samples produces
 *     S[j] = sum of q(a[i]) over s(g0 + i) = j,  j = s(g0) ... s(g0 + n_k - 1)   (int64)
 * The sums are exact integers, so they do not depend on the order of the additions, the
 * tiling, n_channels, the stride or the address: bit-identical from run to run, and a row
 * cut into calls anywhere gives the completed sub-cells of the row given whole.  One
 * launch per call whatever n_channels; a slot with n_k = 0 writes nothing; a call whose
 * counts are all 0 launches nothing.
 * ------------------------------------------------------------------------ */
typedef struct rfa_code rfa_code;

#define RFA_CODE_MAX_CHANNELS 1024             /* n_channels above this: RFA_ERR_INVALID */
#define RFA_CODE_MIN_RATE 8000
#define RFA_CODE_MAX_RATE 384000
#define RFA_CODE_SUBCELLS 8                    /* P: sub-cells per bit */
#define RFA_CODE_WORD_BITS 23

/* Host only, no device: s(g) for 0 <= g <= 2^48.  RFA_ERR_INVALID for a rate outside the range,
 * g outside the limit or a NULL pointer. */
RFA_API int rfa_code_subcell(int32_t sample_rate, int64_t g, int64_t *j);
/* Host only: the 23-bit word of a 9-bit code (0 ... 0x1ff; 023 octal -> 0x763813), bit i of
 * the result being bit i on the air. */
RFA_API int rfa_code_word(int32_t code, uint32_t *word);
/* Host only: the carry arithmetic of one slot and call.  sums[m] are the call's touched
 * sub-cells j0 ... j0 + m - 1, g_end the slot's counter behind the call.  A valid carry
 * (whose carry_j must be j0) is added to sums[0]; where the next sample still falls into the
 * last sub-cell (s(g_end) = j0 + m - 1) that one becomes the carry and is held back.  On
 * return *first = j0 and *count completed sub-cells stand in sums[0 ... *count - 1].  m = 0
 * leaves the carry as it is. */
RFA_API int rfa_code_merge(int32_t sample_rate, int64_t g_end, int64_t j0, int64_t m, int64_t *sums,
                           int32_t *carry_valid, int64_t *carry_j, int64_t *carry_sum, int64_t *first,
                           int64_t *count);

/* 1 <= n_channels <= RFA_CODE_MAX_CHANNELS and a rate in range; arguments are checked before
 * the device is looked for. */
RFA_API int rfa_code_create(int device, int32_t n_channels, int32_t sample_rate, rfa_code **out);
RFA_API int rfa_code_destroy(rfa_code *t);
RFA_API const char *rfa_code_last_error(const rfa_code *t);
RFA_API int rfa_code_get_channels(const rfa_code *t, int32_t *n_channels, int32_t *sample_rate);
/* Slot k's sample counter (k = -1: every slot's) back to 0 and its carry dropped; what an
 * uncollected call holds of the slot is dropped too (its collect reports 0 sub-cells). */
RFA_API int rfa_code_break(rfa_code *t, int32_t k);
/* Every counter to 0, every carry dropped, the last results to 0, no call outstanding. */
RFA_API int rfa_code_reset(rfa_code *t);
/* Device rows audio_stride floats apart, host counts n_audio[n_channels] (what
 * rfa_demod_bank_process returns).  Asynchronous: the call's records go through a ring of
 * pinned entries guarded by events, then the launch, one copy of the sums into pinned memory
 * and an event, all on the handle's stream; the buffers grow on demand.  The carry needs
 * every call collected once: a call while the previous one is uncollected is RFA_ERR_STATE.
 * A count above audio_stride where n_channels > 1, or a NULL row or count array with any
 * count > 0, is RFA_ERR_INVALID; nothing is consumed on an error. */
RFA_API int rfa_code_process(rfa_code *t, const float *audio, size_t audio_stride, const size_t *n_audio);
/* Waits for the last rfa_code_process's event alone, merges the carries and hands out, per
 * slot: the absolute index of the first completed sub-cell, their number, their sums (row k
 * at sums + k * sums_stride), the call's bad count and its sample count; any may be NULL.
 * A number above sums_stride is RFA_ERR_SIZE and the results stay collectable.  Without a
 * call since the last collect it waits for nothing and repeats the values. */
RFA_API int rfa_code_collect(rfa_code *t, int64_t *first, int64_t *count, int64_t *sums, size_t sums_stride,
                             int64_t *bad, int64_t *n);
/* rfa_code_process with host rows, then rfa_code_collect: synchronous. */
RFA_API int rfa_code_process_host(rfa_code *t, const float *audio, size_t audio_stride, const size_t *n_audio,
                                  int64_t *first, int64_t *count, int64_t *sums, size_t sums_stride, int64_t *bad,
                                  int64_t *n);
/* As rfa_ddc_set_stream / _get_stream / _synchronize. */
RFA_API int rfa_code_set_stream(rfa_code *t, void *stream);
RFA_API int rfa_code_get_stream(const rfa_code *t, void **stream);
RFA_API int rfa_code_synchronize(rfa_code *t);

/* ---------------------------------------------------------------------------
 * Audio FIR bank (extension): a real FIR on every bank slot's audio row
 *
 * What follows the demodulators: a slot that opens on its CTCSS tone would hand the
 * listener that tone as a hum under the voice; a high-pass at about 300 Hz removes it
 * (demod.voice_taps).  The reference filters no audio behind its demodulator; the
 * arithmetic is that of its real FIR (dsp/FirFilter.kt:121-163), one slot at a time.
 *
 * Slot k has its own taps t[0 ... T-1] (0 <= T <= RFA_AUDIO_FIR_MAX_TAPS), its own
 * history and its own sample count per call.  With n = n_audio[k] inputs x[0 ... n-1]
 * the call writes n outputs
 *     y[i] = (((+0.0f + t[0] * x[i]) + t[1] * x[i-1]) + ... + t[T-1] * x[i-T+1])
 * every product rounded to float32, every sum rounded to float32, in this order,
 * nothing contracted; x[j], j < 0, is the slot's history.  T = 0 is a pass-through:
 * the output is the input bit for bit, NaN payloads included, without delay.  A
 * non-finite input reaches the T outputs it is a term of, in its own slot only.
 *
 * History: the slot's last RFA_AUDIO_FIR_MAX_TAPS - 1 inputs, on the device, zeros at
 * first, whatever its tap count (pass-through included): new taps need no special
 * case.  A call advances it by the slot's n; a slot with n = 0 keeps it.  A row cut
 * into calls anywhere gives the outputs of the row given whole, bit for bit.
 *
 * One launch per call whatever n_channels: one workgroup per (slot, tile of
 * RFA_AUDIO_FIR_TILE outputs); the history has two buffers per slot and a call writes
 * the one it does not read.  A call whose counts are all 0 launches nothing.
 * ------------------------------------------------------------------------ */
typedef struct rfa_audio_fir rfa_audio_fir;

#define RFA_AUDIO_FIR_MAX_CHANNELS 1024        /* n_channels above this: RFA_ERR_INVALID */
#define RFA_AUDIO_FIR_MAX_TAPS 4096
#define RFA_AUDIO_FIR_TILE 2048                /* outputs of one workgroup */
#define RFA_AUDIO_FIR_NARROW_MAX 512           /* a slot with n up to this takes the narrow path */
/* rfa_audio_fir_plan: the path a slot takes */
#define RFA_AUDIO_FIR_PATH_NONE 0              /* n = 0: the slot's workgroups return at once */
#define RFA_AUDIO_FIR_PATH_COPY 1              /* no taps: bitwise copy */
#define RFA_AUDIO_FIR_PATH_NARROW 2            /* 2 outputs per thread, 2 taps per step */
#define RFA_AUDIO_FIR_PATH_WIDE 3              /* 8 outputs per thread, 4 taps per step */
#define RFA_AUDIO_FIR_PLAN_FIELDS 5            /* tile, lds_bytes, path, outputs per thread, workgroups */

/* Host only, no device: what a call of one slot with num_taps taps and n samples runs:
 * plan[0] RFA_AUDIO_FIR_TILE, [1] the launch's dynamic LDS bytes, [2] the path, [3] outputs
 * per thread (0 on NONE and COPY), [4] the slot's workgroups that do work, ceil(n / tile).
 * RFA_ERR_INVALID for num_taps outside 0 ... RFA_AUDIO_FIR_MAX_TAPS, n above 2^36 or NULL. */
RFA_API int rfa_audio_fir_plan(int32_t num_taps, size_t n, int32_t *plan);
/* Host only: where sample j (0 oldest ... RFA_AUDIO_FIR_MAX_TAPS - 2 newest) of a slot's history
 * comes from after a call of n inputs: *from_input 0 and *index into the history before the
 * call, or *from_input 1 and *index into the call's inputs.  The kernel's own arithmetic.
 * RFA_ERR_INVALID for j outside the history, n above 2^36 or a NULL pointer. */
RFA_API int rfa_audio_fir_history_source(size_t n, int32_t j, int32_t *from_input, size_t *index);

/* 1 <= n_channels <= RFA_AUDIO_FIR_MAX_CHANNELS; arguments are checked before the device
 * is looked for.  Every slot starts as a pass-through with a zero history. */
RFA_API int rfa_audio_fir_create(int device, int32_t n_channels, rfa_audio_fir **out);
RFA_API int rfa_audio_fir_destroy(rfa_audio_fir *f);
RFA_API const char *rfa_audio_fir_last_error(const rfa_audio_fir *f);
RFA_API int rfa_audio_fir_get_channels(const rfa_audio_fir *f, int32_t *n_channels);
/* Slot k's taps from the next call on (num_taps = 0: pass-through; taps may then be NULL); the
 * history stays.  A non-finite tap is RFA_ERR_INVALID and changes nothing.  The upload is
 * ordered on the handle's stream behind every call enqueued so far, through one pinned stage:
 * a set_taps waits until the previous set_taps' upload has been made, so a run of them behind
 * queued calls drains the stream.  The first one after a call waits for nothing. */
RFA_API int rfa_audio_fir_set_taps(rfa_audio_fir *f, int32_t k, const float *taps, int32_t num_taps);
/* *num_taps is slot k's tap count; the taps are copied where capacity holds them (taps may be
 * NULL with capacity 0 to ask for the count). */
RFA_API int rfa_audio_fir_get_taps(const rfa_audio_fir *f, int32_t k, float *taps, size_t capacity,
                                   int32_t *num_taps);
/* Slot k's history (k = -1: every slot's) to zeros, ordered on the stream; the taps stay. */
RFA_API int rfa_audio_fir_reset(rfa_audio_fir *f, int32_t k);
/* Device rows in and out, in_stride / out_stride floats apart, host counts n_audio[n_channels]
 * (what rfa_demod_bank_process returns).  Asynchronous on the handle's stream: the call's
 * records (counts, tap counts, history buffers) go through a ring of pinned entries guarded by
 * events, then one launch.  A steady-state call allocates nothing and waits for nothing.
 * RFA_ERR_INVALID, nothing consumed: a count above either stride where n_channels > 1, a NULL
 * row or count array with any count > 0, input and output ranges that overlap. */
RFA_API int rfa_audio_fir_process(rfa_audio_fir *f, const float *in, size_t in_stride, const size_t *n_audio,
                                  float *out, size_t out_stride);
/* rfa_audio_fir_process with host rows: synchronous. */
RFA_API int rfa_audio_fir_process_host(rfa_audio_fir *f, const float *in, size_t in_stride, const size_t *n_audio,
                                       float *out, size_t out_stride);
/* As rfa_ddc_set_stream / _get_stream / _synchronize. */
RFA_API int rfa_audio_fir_set_stream(rfa_audio_fir *f, void *stream);
RFA_API int rfa_audio_fir_get_stream(const rfa_audio_fir *f, void **stream);
RFA_API int rfa_audio_fir_synchronize(rfa_audio_fir *f);

/* ---------------------------------------------------------------------------
 * Audio resampler bank (extension): every bank slot's audio row to 8 / 16 kHz PCM
 *
 * What follows the audio FIR: loggers, codecs and recognisers want narrow-band s16,
 * not 48 kHz float.  The reference's AudioSink plays float at 48 kHz and resamples
 * nothing; this stage is defined by the text below and checked against its
 * restatement in numpy (tests/audio_rs_ref.py), bit for bit.
 *
 * Handle constants, one set for all slots, fixed at creation: a ratio L / D with
 * 1 <= L <= RFA_AUDIO_RS_MAX_L, L <= D <= RFA_AUDIO_RS_MAX_D and gcd(L, D) = 1, and
 * one real prototype FIR h[0 ... T-1], all finite, T <= RFA_AUDIO_RS_MAX_TAPS, with
 * J = ceil(T / L) taps per phase, 1 <= J <= RFA_AUDIO_RS_MAX_PHASE_TAPS.  L = D = 1
 * may have T = 0: no filter, only the conversion.
 *
 * Per-slot state: a history of the slot's last RFA_AUDIO_RS_HISTORY inputs on the
 * device, zeros at first (two buffers, a call writes the one it does not read, as in
 * the audio FIR bank), and an offset r, 0 <= r < D, on the host, 0 at first: the
 * position of the slot's next output relative to the next input it will receive, in
 * ticks of the rate L * f_in.
 *
 * A call gives slot k n = n_audio[k] inputs x[0 ... n-1].  Its outputs are
 * m = 0, 1, ... while r + m * D < n * L.  Output m has u = r + m * D, input index
 * i = floor(u / L) and phase p = u mod L, and
 *     y = (((+0.0f + h[p] * x[i]) + h[p+L] * x[i-1]) + ... + h[p+(J-1)L] * x[i-J+1])
 * Taps at or beyond T count as +0.0f and are still multiplied and added.  Every
 * product and every sum is rounded to float32 in this order, nothing contracted;
 * x[j], j < 0, is the history.  After the call r <- r + n_out * D - n * L and the
 * history advances by n.  A slot with n = 0 does nothing and keeps everything.  So
 * n_out = ceil((n * L - r) / D) for n * L > r, else 0; a stream cut into calls anywhere
 * gives the outputs of the stream given whole, bit for bit, with the same total count;
 * with T = 0, y = x bitwise.
 *
 * PCM: v = y * 32768.0f (exact); NaN -> 0; v >= 32767 -> 32767; v <= -32768 -> -32768;
 * otherwise (int16_t)rintf(v), ties to even.  A PCM value q read back through the
 * RFA_IN_S16LE conversion is exactly q / 32768.
 *
 * One launch per call whatever n_channels: a grid of (output tiles of the longest row,
 * n_channels) workgroups.  A call whose counts are all 0 launches nothing.
 * ------------------------------------------------------------------------ */
typedef struct rfa_audio_rs rfa_audio_rs;

#define RFA_AUDIO_RS_MAX_CHANNELS 1024         /* n_channels above this: RFA_ERR_INVALID */
#define RFA_AUDIO_RS_MAX_L 160
#define RFA_AUDIO_RS_MAX_D 1024
#define RFA_AUDIO_RS_MAX_TAPS 16384            /* T */
#define RFA_AUDIO_RS_MAX_PHASE_TAPS 4096       /* J = ceil(T / L) */
#define RFA_AUDIO_RS_HISTORY 4095              /* inputs a slot keeps between calls */
#define RFA_AUDIO_RS_MAX_TILE 1024             /* outputs of one workgroup, at most */
/* rfa_audio_rs_plan: the path a slot takes */
#define RFA_AUDIO_RS_PATH_NONE 0               /* n = 0: the slot's workgroups return at once */
#define RFA_AUDIO_RS_PATH_CONVERT 1            /* T = 0: the conversion alone */
#define RFA_AUDIO_RS_PATH_DECIMATE 2           /* L = 1: one tap row for all outputs, samples de-interleaved by D */
#define RFA_AUDIO_RS_PATH_POLYPHASE 3          /* L > 1: every output reads its own phase row */
#define RFA_AUDIO_RS_PLAN_FIELDS 5             /* tile, lds_bytes, path, outputs per thread, workgroups */

/* Host only, no device: the call rule, the kernel launch's own arithmetic.  A slot at offset r
 * given n inputs writes *n_out outputs and is then at offset *r_next.  No overflow for n up to
 * 2^36.  RFA_ERR_INVALID for a ratio outside the limits above, r outside 0 ... D-1, n above
 * 2^36 or a NULL pointer. */
RFA_API int rfa_audio_rs_counts(int32_t L, int32_t D, int32_t r, size_t n, size_t *n_out, int32_t *r_next);
/* Host only: ceil(n * L / D), the most outputs any call of n inputs writes; 0 for a ratio
 * outside the limits or n above 2^36. */
RFA_API size_t rfa_audio_rs_max_outputs(int32_t L, int32_t D, size_t n);
/* Host only: what a call of one slot at offset 0 with n inputs runs: plan[0] the output tile of
 * this ratio and tap count (at most RFA_AUDIO_RS_MAX_TILE; smaller where the tile's inputs would
 * not fit the LDS), [1] the launch's dynamic LDS bytes, [2] the path, [3] outputs per thread
 * (0 on NONE), [4] the slot's workgroups that do work.  RFA_ERR_INVALID for what
 * rfa_audio_rs_create refuses, n above 2^36 or NULL. */
RFA_API int rfa_audio_rs_plan(int32_t L, int32_t D, int32_t num_taps, size_t n, int32_t *plan);

/* 1 <= n_channels <= RFA_AUDIO_RS_MAX_CHANNELS and the limits above; a non-finite tap, NULL
 * taps with num_taps > 0 or a NULL out is RFA_ERR_INVALID.  Arguments are checked before the
 * device is looked for.  Every slot starts with a zero history at offset 0. */
RFA_API int rfa_audio_rs_create(int device, int32_t n_channels, int32_t L, int32_t D, const float *taps,
                                int32_t num_taps, rfa_audio_rs **out);
RFA_API int rfa_audio_rs_destroy(rfa_audio_rs *s);
RFA_API const char *rfa_audio_rs_last_error(const rfa_audio_rs *s);
RFA_API int rfa_audio_rs_get_channels(const rfa_audio_rs *s, int32_t *n_channels);
RFA_API int rfa_audio_rs_get_ratio(const rfa_audio_rs *s, int32_t *L, int32_t *D);
/* *num_taps is T; the taps are copied where capacity holds them (taps may be NULL with
 * capacity 0 to ask for the count). */
RFA_API int rfa_audio_rs_get_taps(const rfa_audio_rs *s, float *taps, size_t capacity, int32_t *num_taps);
/* Slot k's history to zeros, ordered on the stream, and its offset to 0 (k = -1: every slot). */
RFA_API int rfa_audio_rs_reset(rfa_audio_rs *s, int32_t k);
/* Slot k's offset r as of the calls made so far. */
RFA_API int rfa_audio_rs_get_offset(const rfa_audio_rs *s, int32_t k, int32_t *r);
/* Device rows: in, in_stride floats apart, host counts n_audio[n_channels]; out_f32 rows
 * f32_stride floats apart and out_s16 rows s16_stride int16 apart.  Either output may be NULL,
 * not both.  n_out[n_channels] (host, may be NULL) is filled before the launch, from the rule
 * above.  Asynchronous on the handle's stream: the call's records (counts, offsets, history
 * buffers) go through a ring of pinned entries guarded by events, then one launch.  A
 * steady-state call allocates nothing and waits for nothing.  Any 2-byte-aligned out_s16 and
 * any s16_stride work: the kernel stores int16 one at a time.
 * RFA_ERR_INVALID, nothing consumed: an input count above in_stride or an output count above an
 * output's stride where n_channels > 1, a NULL input row or both outputs NULL with work to do,
 * a NULL count array, an output range that overlaps the input or the other output, a float
 * pointer off a 4-byte or an int16 pointer off a 2-byte boundary.
 * RFA_ERR_UNSUPPORTED, nothing consumed: the taps' LDS image is above 64 KiB (rfa_audio_rs_plan
 * reports it) and the device did not grant the launch that much. */
RFA_API int rfa_audio_rs_process(rfa_audio_rs *s, const float *in, size_t in_stride, const size_t *n_audio,
                                 float *out_f32, size_t f32_stride, int16_t *out_s16, size_t s16_stride,
                                 size_t *n_out);
/* rfa_audio_rs_process with host rows: synchronous. */
RFA_API int rfa_audio_rs_process_host(rfa_audio_rs *s, const float *in, size_t in_stride, const size_t *n_audio,
                                      float *out_f32, size_t f32_stride, int16_t *out_s16, size_t s16_stride,
                                      size_t *n_out);
/* As rfa_ddc_set_stream / _get_stream / _synchronize. */
RFA_API int rfa_audio_rs_set_stream(rfa_audio_rs *s, void *stream);
RFA_API int rfa_audio_rs_get_stream(const rfa_audio_rs *s, void **stream);
RFA_API int rfa_audio_rs_synchronize(rfa_audio_rs *s);

/* ---------------------------------------------------------------------------
 * Audio IIR bank (extension): second-order recursive sections on every bank slot's audio row
 *
 * What an NFM receiver ends in, a 6 dB / octave de-emphasis, and a tone strip that a packet
 * can afford: an 8th-order Chebyshev II high-pass (demod.tone_strip_sections) in place of
 * the 1309-tap FIR.  The reference filters no audio behind its demodulator and has no
 * recursive filter: no entry of this section has a counterpart there.  The stage is defined
 * by the text below and checked against its restatement in numpy (tests/audio_iir_ref.py),
 * bit for bit.
 *
 * Slot k has S sections, 0 <= S <= RFA_AUDIO_IIR_MAX_SECTIONS, each five float32
 * coefficients (b0, b1, b2, a1, a2) with a0 = 1; a first-order section has b2 = a2 = 0.
 * S = 0 copies the row bit for bit, NaN payloads included.  Section q's input is section
 * q-1's output, section 0's the row.  Every product and every sum below is rounded to
 * float32, in the written order, nothing contracted.
 *
 * B = RFA_AUDIO_IIR_BLOCK.  A slot counts the samples it has consumed since its last reset
 * or set_sections, a = 0, 1, ...; sample a lies in block a div B at offset i = a mod B.
 * One step (transposed direct form II) with state (z1, z2) and input u:
 *     v = (b0*u) + z1;   z1' = ((b1*u) - (a1*v)) + z2;   z2' = (b2*u) - (a2*v)
 * Per section and block j with block-start state s0_j (two floats, s0_0 = (0, 0)):
 *   zero-state response: zs[i] and the running state z are that step started from
 *     z = (0, 0) at i = 0 and run over the block's inputs;
 *   output:      y[i] = zs[i] + ((G[i][0]*s0_j[0]) + (G[i][1]*s0_j[1]))
 *   next block:  s0_{j+1}[r] = ((P[r][0]*s0_j[0]) + (P[r][1]*s0_j[1])) + z_end[r], r = 0, 1,
 *     z_end being z after the block's B-th step.
 * Tables per section, computed in double from the float32 coefficients widened and rounded
 * once to float32: A = [[-a1, 1], [-a2, 0]], R_0 = I, R_{i+1} = R_i A with every element
 * (x0*A0c) + (x1*A1c) in that order; G[i] is the first row of R_i, i = 0 ... B-1, P = R_B.
 *
 * Between calls a slot carries, per section, s0 and the running z of its incomplete block,
 * and a mod B.  A call that ends inside a block leaves these and the next call goes on from
 * them, so a row cut into calls anywhere gives the bits of the row given whole.  A
 * non-finite input makes the slot's state non-finite from its block on, until the slot is
 * reset; other slots are untouched.
 *
 * One launch per call whatever n_channels: one workgroup per slot, which walks the row in
 * chunks of RFA_AUDIO_IIR_CHUNK_BLOCKS blocks staged in LDS.  A slot with n = 0 keeps
 * everything; a call whose counts are all 0 launches nothing.
 * ------------------------------------------------------------------------ */
typedef struct rfa_audio_iir rfa_audio_iir;

#define RFA_AUDIO_IIR_MAX_CHANNELS 1024        /* n_channels above this: RFA_ERR_INVALID */
#define RFA_AUDIO_IIR_MAX_SECTIONS 8
#define RFA_AUDIO_IIR_BLOCK 128                /* B */
#define RFA_AUDIO_IIR_CHUNK_BLOCKS 256         /* blocks a workgroup stages at a time, one lane each */
/* rfa_audio_iir_plan: the path a slot takes */
#define RFA_AUDIO_IIR_PATH_NONE 0              /* n = 0: the slot's workgroup returns at once */
#define RFA_AUDIO_IIR_PATH_COPY 1              /* no sections: bitwise copy */
#define RFA_AUDIO_IIR_PATH_BLOCKED 2           /* the blocked recurrence */
#define RFA_AUDIO_IIR_PLAN_FIELDS 6            /* B, blocks per chunk, lds_bytes, path, chunks, blocks touched */

/* Host only, no device, no counterpart in the reference: the library's own tables of a section
 * with these a1, a2: G[RFA_AUDIO_IIR_BLOCK][2] and P[4] = P[0][0], P[0][1], P[1][0], P[1][1].
 * RFA_ERR_INVALID, nothing written: a1 or a2 not finite or outside the stability triangle
 * (|a2| < 1 and |a1| < 1 + a2), or a NULL pointer. */
RFA_API int rfa_audio_iir_tables(float a1, float a2, float *G, float *P);
/* Host only, no counterpart in the reference: what a call of one slot with num_sections sections,
 * n samples and a mod B = a_mod_B runs: plan[0] RFA_AUDIO_IIR_BLOCK, [1] RFA_AUDIO_IIR_CHUNK_BLOCKS,
 * [2] the launch's dynamic LDS bytes (0 on NONE and COPY; above 64 KiB for a full chunk: the
 * create entry raises the kernel's limit), [3] the path, [4] the chunks the workgroup walks
 * (0 on NONE and COPY), [5] the blocks the call touches, ceil((a_mod_B + n) / B).
 * RFA_ERR_INVALID for num_sections outside 0 ... RFA_AUDIO_IIR_MAX_SECTIONS, a_mod_B outside
 * 0 ... B-1, n above 2^36 or NULL. */
RFA_API int rfa_audio_iir_plan(int32_t num_sections, size_t n, int32_t a_mod_B, int32_t *plan);
/* Host only, no counterpart in the reference: *next = (a_mod_B + n) mod B, a slot's offset in its
 * block after a call of n samples.  RFA_ERR_INVALID as rfa_audio_iir_plan. */
RFA_API int rfa_audio_iir_carry_after(size_t n, int32_t a_mod_B, int32_t *next);

/* 1 <= n_channels <= RFA_AUDIO_IIR_MAX_CHANNELS; arguments are checked before the device is
 * looked for.  Every slot starts as a pass-through with a zero carry.  No counterpart in the
 * reference, as for every entry below. */
RFA_API int rfa_audio_iir_create(int device, int32_t n_channels, rfa_audio_iir **out);
RFA_API int rfa_audio_iir_destroy(rfa_audio_iir *f);
RFA_API const char *rfa_audio_iir_last_error(const rfa_audio_iir *f);
RFA_API int rfa_audio_iir_get_channels(const rfa_audio_iir *f, int32_t *n_channels);
/* Slot k's sections from the next call on: coeffs[num_sections][5] as (b0, b1, b2, a1, a2);
 * num_sections = 0 is the pass-through and coeffs may then be NULL.  The slot's carry is zeroed
 * and its block grid starts again at the next sample.  A coefficient that is not finite or a
 * section outside the stability triangle (|a2| < 1 and |a1| < 1 + a2) is RFA_ERR_INVALID and
 * changes nothing.  The tables are uploaded on the handle's stream behind every call enqueued
 * so far, through one pinned stage, as rfa_audio_fir_set_taps uploads taps.  "Changes nothing"
 * covers argument errors: after RFA_ERR_HIP the slot's tables and carry on the device are
 * undefined until a set_sections for that slot succeeds (get_sections still reports the old ones). */
RFA_API int rfa_audio_iir_set_sections(rfa_audio_iir *f, int32_t k, const float *coeffs, int32_t num_sections);
/* *num_sections is slot k's S.  coeffs NULL asks for the count alone; otherwise capacity, in
 * sections, must hold them: below S it is RFA_ERR_INVALID with *num_sections set and nothing
 * copied. */
RFA_API int rfa_audio_iir_get_sections(const rfa_audio_iir *f, int32_t k, float *coeffs, size_t capacity,
                                       int32_t *num_sections);
/* Slot k's carry (k = -1: every slot's) to zeros, ordered on the stream, and its block grid to
 * the next sample; the sections stay. */
RFA_API int rfa_audio_iir_reset(rfa_audio_iir *f, int32_t k);
/* Device rows in and out, in_stride / out_stride floats apart, host counts n_audio[n_channels]
 * (what rfa_demod_bank_process returns).  Asynchronous on the handle's stream: the call's
 * records (counts, section counts, offsets) go through a ring of pinned entries guarded by
 * events, then one launch.  A steady-state call allocates nothing and waits for nothing.
 * RFA_ERR_INVALID, nothing consumed: a count above either stride where n_channels > 1, a NULL
 * row or count array with any count > 0, input and output ranges that overlap. */
RFA_API int rfa_audio_iir_process(rfa_audio_iir *f, const float *in, size_t in_stride, const size_t *n_audio,
                                  float *out, size_t out_stride);
/* rfa_audio_iir_process with host rows: synchronous. */
RFA_API int rfa_audio_iir_process_host(rfa_audio_iir *f, const float *in, size_t in_stride, const size_t *n_audio,
                                       float *out, size_t out_stride);
/* As rfa_ddc_set_stream / _get_stream / _synchronize. */
RFA_API int rfa_audio_iir_set_stream(rfa_audio_iir *f, void *stream);
RFA_API int rfa_audio_iir_get_stream(const rfa_audio_iir *f, void **stream);
RFA_API int rfa_audio_iir_synchronize(rfa_audio_iir *f);

#ifdef __cplusplus
}
#endif

#endif /* RFA_H */
